"""GPU (-m gpu): the pruned matrix-core sweeps of new frames against a LARGE reference -- pop_against_kernel
(calculate_populations_against(..., variant="cross_pruned")) and nn_against_kernel (nearest_reference(..., pruned=True))
-- on the paths the small references of test_gpu_cross_pruned.py / test_gpu_cross_nn_pruned.py never enter:
  A  more than one scan round of kListCap = 512 reference tiles in one share (512, 513, 1024, 1025 tiles), the work
     before, behind and across the round boundary, nn and hd in different rounds, a tie across the boundary;
  B  2 .. 64 reference shares of the population sweep (DC_SHARE_FLOOR = 8), and several shares with several rounds each;
  C  every pair in the guard band (16 band elements per lane and tile: the queue flushes in mid-epilogue);
  D  a duplicated reference whose copies lie in all tiles of both rounds;
  E  the last reference the pruned kernels take: 2^24 padded positions, the partners at the end of the order.
One width per class of kernel instance (tests/crossbigref.py: D = 3 full chains, 10 and 16 the early-out with one and two
coarse MFMAs, 24 single buffer).  The referee is the probe's canonical d2 (crossref.block_d2 in pieces, expect_pops,
expect_nn, same_nn: populations equal as integers, index and d2 bits equal; numpy's float32 in case E), never the GPU,
and after every call the counters say that the pruned kernel answered.  DC_SHARE_FLOOR is read once per process, so the
runs under it are fresh child processes.  The premises of the built cases: tests/test_cross_big_cases.py.

Measured on one MI355X: 37 tests in 36 s, the slowest (a child process) 3.0 s; case E: see its docstring."""
import os
import subprocess
import sys

import numpy as np
import pytest

import crossbigref as cb
import crossprunedref as cp
from crossref import block_d2, expect_nn, expect_pops, gpu, host, same_nn, sets

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


def device():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def nn_info(dens):
    return dens.evaluated_tiles_nearest_reference(device())


def check_pops(dens, Q, R, radii, exp, what, i_from=0, i_to=None, out=None):
    """populations equal as integers, and the pruned sweep answered"""
    got = dens.calculate_populations_against(gpu(Q), gpu(R), radii, i_from, len(Q) if i_to is None else i_to, variant=V, out=out)
    bad = np.argwhere(host(got) != exp)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), host(got)[tuple(bad[0])], exp[tuple(bad[0])])
    tiles, mfma = dens.evaluated_tiles_against(device())
    assert tiles > 0 and mfma > 0, (what, tiles, mfma)
    return got


def check_nn(dens, Q, R, fe_q, fe_r, d2, what, shares=None, nn_only=True):
    """index and d2 bits equal with free energies and again for nn alone, and the pruned kernel answered"""
    q, r = gpu(Q), gpu(R)
    calls = [(fe_q, fe_r)] + ([(None, None)] if nn_only else [])
    for fq, fr in calls:
        exp = expect_nn(d2, fq, fr)
        got = dens.nearest_reference(q, r, None if fq is None else gpu(fq), None if fr is None else gpu(fr), pruned=True)
        same_nn(got, exp, (what, "nn only" if fq is None else "fe"))
        tiles, mfma, n_shares = nn_info(dens)
        assert tiles > 0 and mfma > 0, (what, tiles, mfma)
        if shares is not None:
            assert shares(n_shares), (what, n_shares)


class Collect:
    """runs every case of a programme and reports all that failed, not only the first"""

    def __init__(self):
        self.failed = []

    def run(self, f, *args, **kw):
        try:
            f(*args, **kw)
        except AssertionError as e:
            self.failed.append(str(e)[:400])

    def done(self):
        assert not self.failed, (len(self.failed), self.failed)


# ---- A: round boundaries ----------------------------------------------------------------------------------------------
def nn_rounds_programme(dens, probe, D, n_r):
    all_cases = Collect()
    for layout in cb.A_LAYOUTS[n_r]:
        c = cb.case_a(D, n_r, layout)
        Q, R = c["Q"], c["R"]
        d2 = cb.big_d2(probe, Q, R)
        fe_q, fe_r = cb.rand_fe(len(Q), n_r, D)
        all_cases.run(check_nn, dens, Q, R, fe_q, fe_r, d2, ("A", D, n_r, layout), lambda n: n == 1)
        if c["tie"]:
            fq, fr = cb.tie_fe_across(len(Q), n_r, *c["tie"])
            all_cases.run(check_nn, dens, Q, R, fq, fr, d2, ("A tie", D, n_r, layout), nn_only=False)
    all_cases.done()


@pytest.mark.parametrize("n_r", cb.A_SIZES)
@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_neighbours_across_scan_rounds(dens, probe, D, n_r):
    """one share (the sweep's own floor of 900 tiles): rounds of 512 tiles, the partners before, behind and on both sides
    of the boundary, and the same d2 in tile 511 and tile 512 with the lower index in the later one"""
    nn_rounds_programme(dens, probe, D, n_r)


@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_nn_and_hd_in_different_rounds(dens, probe, D):
    """A4: the nearest frame in one round, the only frame of lower free energy in the other"""
    for far_round in (0, 1):
        Q, R, fe_q, fe_r, special = cb.case_a4(D, far_round)
        d2 = cb.big_d2(probe, Q, R)
        assert (expect_nn(d2, fe_q, fe_r)[2] == special).all()
        check_nn(dens, Q, R, fe_q, fe_r, d2, ("A4", D, far_round), lambda n: n == 1, nn_only=False)


def pop_rounds_programme(dens, probe, D):
    """(in a child under DC_SHARE_FLOOR = 2000: one share) every layout of every size, each radius alone and all three"""
    all_cases = Collect()
    for n_r in cb.A_SIZES:
        for layout in cb.A_LAYOUTS[n_r]:
            c = cb.case_a(D, n_r, layout)
            d2 = cb.big_d2(probe, c["Q"], c["R"])
            all_cases.run(check_pops, dens, c["Q"], c["R"], cb.A_RADII, expect_pops(d2, cb.A_RADII), ("A", D, n_r, layout))
            all_cases.run(check_pops, dens, c["Q"], c["R"], cb.A_RADII[:1], expect_pops(d2, cb.A_RADII[:1]),
                          ("A one radius", D, n_r, layout))
    if D in (3, 10):
        all_cases.run(duplicates_pops, dens, probe, D)
    all_cases.done()


# ---- D: duplicates across rounds -----------------------------------------------------------------------------------------
def duplicates_pops(dens, probe, D):
    Q, R, _ = cb.case_d(D)
    d2 = cb.big_d2(probe, Q, R)
    radii = [0.05, 0.3, 0.6]
    exp = expect_pops(d2, radii)
    assert (exp[0][:150] >= 400).all()
    check_pops(dens, Q, R, radii, exp, ("D", D))


@pytest.mark.parametrize("D", [3, 10])
def test_duplicated_reference_across_rounds(dens, probe, D):
    """nn is the lowest index of 400 copies that lie in all tiles of both rounds (the populations of this case: the
    child of test_populations_across_scan_rounds)"""
    Q, R, which = cb.case_d(D)
    d2 = cb.big_d2(probe, Q, R)
    fe_q, fe_r = cb.rand_fe(len(Q), len(R), D)
    check_nn(dens, Q, R, fe_q, fe_r, d2, ("D", D), lambda n: n == 1)


# ---- child processes -------------------------------------------------------------------------------------------------------
CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import test_gpu_cross_pruned_big as t
getattr(t, sys.argv[2])(dens, Probe(capi.CANON_ORDER), *[int(a) for a in sys.argv[3:]])
print("ok")
"""


def run_child(env, *args):
    env = dict(os.environ, **env)
    env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, *[str(a) for a in args]], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_populations_across_scan_rounds(D):
    """DC_SHARE_FLOOR = 2000, above every tile count of case A: one share, so the rounds of 512 tiles are real"""
    run_child({"DC_SHARE_FLOOR": "2000"}, "pop_rounds_programme", D)


# ---- B: population shares ------------------------------------------------------------------------------------------------
def pop_shares_programme(dens, probe, D):
    import torch
    for n_q, n_r in cb.B_SHAPES:
        Q, R = sets(D, n_q, n_r, seed=D + n_r)
        d2 = cb.big_d2(probe, Q, R)
        r0 = 0.2 if D <= 10 else float(0.08 * np.sqrt(2.0 * D))
        radii = [0.5 * r0, r0, 2.0 * r0]
        exp = expect_pops(d2, radii)
        assert (exp > 0).any(axis=1).all()
        # the same call twice into the same tensor (ascending radii: the library writes into it directly), then a row
        # range in it: the caller's zero-fill makes the atomic merge right, and the rows outside stay 0
        out = torch.full((3, n_q), 12345, dtype=torch.int32, device="cuda")
        check_pops(dens, Q, R, radii, exp, ("B", D, n_r), out=out)
        check_pops(dens, Q, R, radii, exp, ("B again", D, n_r), out=out)
        i_from, i_to = n_q // 5, n_q - n_q // 7
        part = expect_pops(d2, radii, i_from, i_to)
        assert (part[:, :i_from] == 0).all() and (part[:, i_to:] == 0).all() and (part > 0).any()
        check_pops(dens, Q, R, radii, part, ("B range", D, n_r), i_from, i_to, out=out)
    # exact radius ties in several shares: the lattice trio in one call and each alone
    g, (r_at, r_above, r_below) = cp.lattice_radii()
    Q, R = cp.lattice_sets(D, g)
    d2 = block_d2(probe, Q, R)
    for radii in ([r_above, r_below, r_at], [r_at], [r_above], [r_below]):
        check_pops(dens, Q, R, radii, expect_pops(d2, radii), ("B lattice", D, radii))
    every_pair_programme(dens, probe, D, sizes=[2048], shares=lambda n: n > 1)


@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_population_shares(D):
    """DC_SHARE_FLOOR = 8: 16 and 64 shares (tests/test_cross_big_cases.py test_share_counts), a last partial tile, a tile
    count that is no multiple of the share count, three radii, a row range, the same output twice, exact ties; and
    case C once more, its ties settled across shares"""
    run_child({"DC_SHARE_FLOOR": str(cb.B_FLOOR)}, "pop_shares_programme", D)


def joined_programme(dens, probe):
    """DC_SHARE_FLOOR = 600, 40 000 reference rows = 1250 tiles: two shares of 625 tiles, two rounds each, both sweeps"""
    for D in cb.CLASS_WIDTHS:
        Q, R = sets(D, 300, cb.JOIN_ROWS, seed=D)
        d2 = cb.big_d2(probe, Q, R)
        r0 = 0.2 if D <= 10 else float(0.08 * np.sqrt(2.0 * D))
        radii = [0.5 * r0, r0, 2.0 * r0]
        exp = expect_pops(d2, radii)
        assert (exp > 0).any(axis=1).all()
        check_pops(dens, Q, R, radii, exp, ("joined", D))
        fe_q, fe_r = cb.rand_fe(len(Q), len(R), D)
        check_nn(dens, Q, R, fe_q, fe_r, d2, ("joined", D), lambda n: n > 1)


def test_several_shares_of_several_rounds():
    run_child({"DC_SHARE_FLOOR": str(cb.JOIN_FLOOR)}, "joined_programme")


# ---- C: every pair in the band ---------------------------------------------------------------------------------------------
def every_pair_programme(dens, probe, D, sizes=cb.C_SIZES, shares=None):
    for n_r in sizes:
        Q, R, g, (r_at, r_above, r_below) = cb.case_c(D, n_r)
        d2 = block_d2(probe, Q, R)
        for radii in ([r_below], [r_at], [r_above], [r_below, r_at, r_above]):
            exp = expect_pops(d2, radii)
            check_pops(dens, Q, R, radii, exp, ("C", D, n_r, radii))
        assert (exp[0] == 0).all() and (exp[1] == 0).all() and (exp[2] == n_r).all()   # strict '<'
        for where in ("first", "middle", "last"):
            fe_q, fe_r, k0 = cb.c_fe(n_r, where)
            assert (expect_nn(d2, fe_q, fe_r)[2] == k0).all()
            check_nn(dens, Q, R, fe_q, fe_r, d2, ("C", D, n_r, where), shares)


@pytest.mark.parametrize("D", cb.CLASS_WIDTHS)
def test_every_pair_in_the_band(dens, probe, D):
    """n_r copies of one point, 192 queries all exactly g / 8 from it: every element of every accumulator is a band pair
    (populations) or a tie (neighbours: nn is index 0, hd the lowest index of lower free energy, in the first, a middle
    and the last tile of the order)"""
    every_pair_programme(dens, probe, D)


# ---- E: the last reference that is taken -------------------------------------------------------------------------------------
def last_reference_programme(dens, probe, n_r):
    import torch
    Q, R, fe_q, fe_r = cb.case_e(n_r)
    radii, _ = cb.e_radii(Q, R)
    pops, exp, _ = cb.e_expect(Q, R, fe_q, fe_r, radii)
    q, r = gpu(Q), gpu(R)
    try:
        got = dens.calculate_populations_against(q, r, radii, variant=V)
        assert (host(got) == pops).all(), np.argwhere(host(got) != pops)[:5]
        tiles, mfma = dens.evaluated_tiles_against(device())
        assert tiles > 0 and mfma > 0
        dens._cross_pruned_workspaces.clear()
        same_nn(dens.nearest_reference(q, r, gpu(fe_q), gpu(fe_r), pruned=True), exp, ("E", n_r))
        tiles, mfma, n_shares = nn_info(dens)
        assert tiles > 0 and mfma > 0 and n_shares >= 1
    finally:
        dens._cross_pruned_workspaces.clear()
        dens._nearest_pruned_workspaces.clear()
        del q, r
        torch.cuda.empty_cache()


@pytest.mark.parametrize("n_r", cb.E_SIZES)
def test_the_last_reference_that_is_taken(n_r):
    """2^24 padded reference positions (n_r = 2^24, and 2^24 - 31 with a last partial tile): the pruned kernels answer --
    unlike at 2^24 + 1 -- and the band pairs and candidates they queue sit at positions with the top bits set.  D = 1,
    refereed by numpy's float32 (q - r)^2 (tests/test_cross_big_cases.py: equal to the probe's d2 there), radii on, one
    ulp above and one ulp below the distance of an actual pair.  In a child process of its own: its workspaces of
    several GB come and go without touching the device memory of the process that runs the rest of the suite.
    Measured on one MI355X: 2.6 s and 3.0 s with the child's start-up, against 3.1 s of test_more_than_2_24_references
    (2^24 + 1) on the same machine: about the same, so both sizes stay."""
    run_child({}, "last_reference_programme", n_r)
