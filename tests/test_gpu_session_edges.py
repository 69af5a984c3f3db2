"""GPU (-m gpu): resident sessions (dc_hip_session_*, clustering_amd/csrc/dc_session.hip) and dc_hip_density_all in every
call order and at their edges, held to the probe's canonical d2 matrix (tests/sessionref.py) and never to the call-by-call
GPU path, which runs the same kernels.

  orders      one device, 10 and 24 columns: populations (fetched or not), free energies of an index or handed in,
              neighbours, pair lists, forests and populations again in the orders of sessionref.ORDERS; every output
              against the referee over all rows
  who         after every population and neighbour call dc_hip_session_counters must show that the pruned matrix-core
              sweep answered (evaluated tiles > 0), whatever ran before -- or, for flagged data, wide rows and NaN free
              energies, that it did not (0 tiles)
  refusals    calls the state does not allow come back as DC_ERR_INVALID_ARGUMENT with a message, and the session
              answers the next valid call with the referee's values
  counts      1, 9, 2, 17 and 1 radii in one session (the resident array grows), unsorted, with 0, NaN, inf, 1e20
  outputs     every host output pointer NULL by turns
  devices     2, 3 and 5 "devices" on the one GPU (DC_SESSION_ALLOW_DUPLICATE_DEVICES=1, host merge), both neighbour
              merges, 0 .. 2000 rows (devices without a query group), 3 .. 70 columns, flagged data, free energies
              with ties, signed zeros, inf and NaN
  two         two sessions open at once, calls interleaved with each other and with call-by-call sweeps
  all         dc_hip_density_all with every argument set
  rccl        ONE child process: the reduced programme over a one-rank RCCL communicator, both neighbour merges

Everything but `rccl` runs in this process on lattices of at most 2500 rows.  A session call that returns DC_ERR_HIP ends
the run (sessionref.Flow.call)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sessionref as S
from graphref import rank_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    yield density
    log("sessions opened in this process:", S.OPENED[0], "-- child processes: at most 1 (the one-rank RCCL communicator)")


@pytest.fixture(scope="module")
def probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


@pytest.fixture(scope="module")
def one(probe, oracle):
    """the one-device cases: D -> (Ref, radii), computed once and left unchanged"""
    cache = {}

    def get(D):
        if D not in cache:
            name, kind, n, d, seed = S.ONE_DEVICE[D]
            ref = S.Ref(probe, oracle, S.data(kind, n, d, seed))
            cache[D] = (ref, S.radii_of(ref), name)
        return cache[D]
    return get


def log(*a):
    print("session-edges:", *a, flush=True)


# ---- 1. call orders ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", sorted(S.ONE_DEVICE))
@pytest.mark.parametrize("order", sorted(S.ORDERS))
def test_call_orders(dens, one, order, D):
    ref, R, name = one(D)
    f = S.open_flow(dens, ref, f"{name}: {order}", R=R, n_devices=1)
    with f.s:
        assert f.s.n_devices == 1 and f.s.merge_mode == 0
        f.run(S.ORDERS[order][0])


@pytest.mark.parametrize("n", S.TINY_ROWS)
def test_tiny_sessions(dens, probe, oracle, n):
    """0, 1, 2, 31, 33 and 37 rows on one device: every order that needs no tie radii of the data's own"""
    for D in (3, 24):
        ref = S.Ref(probe, oracle, S.data("lattice", n, D, 300 + n))
        R = S.radii_of(ref)
        for order in ("whole flow twice", "forest, pairs, populations", "the lumping flow"):
            f = S.open_flow(dens, ref, f"tiny n={n} D={D}: {order}", R=R, n_devices=1)
            with f.s:
                f.run(S.ORDERS[order][0])


def test_set_free_energies_of_no_rows_takes_a_null_pointer(dens, probe, oracle):
    """every entry point accepts a session of 0 rows with NULL arrays; a NULL array for rows that exist is refused"""
    from clustering_amd import capi
    for n in (0, 5):
        ref = S.Ref(probe, oracle, S.data("lattice", n, 3, 1))
        f = S.open_flow(dens, ref, f"null free energies, {n} rows", R=S.radii_of(ref), n_devices=1)
        with f.s:
            rc = capi.lib.dc_hip_session_set_free_energies(f.s._h, None)
            if n == 0:
                assert rc == capi.DC_OK, capi.lib.dc_hip_last_error()
                assert capi.lib.dc_hip_session_populations(f.s._h, None, 0, None) == capi.DC_OK
                f.nn()
            else:
                assert rc == capi.DC_ERR_INVALID_ARGUMENT and capi.lib.dc_hip_last_error().strip()
                f.refused(f.s.nearest_neighbors)      # (nothing became resident)
                f.set_fe("continuous")
                f.nn()


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------
def _refusal_nn_without_fe(f):
    f.refused(f.s.nearest_neighbors)
    f.pops(f.R["multi3"])
    f.refused(f.s.nearest_neighbors)          # (populations alone are no free energies)
    f.fe(1)
    f.nn()


def _refusal_nn_after_populations(f):
    f.pops(f.R["multi3"])
    f.fe(0)
    f.pops(f.R["one"], fetch=False)           # drops the free energies
    f.refused(f.s.nearest_neighbors)
    f.fe(0)
    f.nn()


def _refusal_index(f):
    f.refused(f.s.free_energies, 0)           # nothing resident yet
    f.pops(f.R["multi3"])
    f.refused(f.s.free_energies, 3)
    f.refused(f.s.free_energies, 2 ** 40)
    f.fe(2)
    f.nn()
    f.pops(f.R["one"])                        # fewer radii than before: index 1 is no longer resident
    f.refused(f.s.free_energies, 1)
    f.fe(0)
    f.nn()


def _refusal_fe_after_pairs(f):
    f.pops(f.R["multi3"])
    f.pairs(f.R["r2"]["above"])
    f.refused(f.s.free_energies, 0)
    f.pops(f.R["multi3"])
    f.fe(1)
    f.nn()


def _refusal_fe_after_forest(f):
    f.pops(f.R["multi3"])
    f.fe(1)
    f.forest(f.R["r2"]["above"], rank_of("random", f.ref.n))
    f.refused(f.s.free_energies, 0)
    f.nn()                                    # (the free energies of before the forest)
    f.pops(f.R["one"])
    f.fe(0)
    f.nn()


def _refusal_rank(f):
    n = f.ref.n
    f.pops(f.R["multi3"])
    f.fe(0)
    twice = rank_of("identity", n)
    twice[7] = twice[8]
    beyond = rank_of("reversed", n)
    beyond[n // 2] = n
    for rank in (twice, beyond):
        f.refused(f.s.radius_forest, f.R["r2"]["above"], rank)
    f.fe(2)                                   # a refused forest has not touched the resident populations
    f.nn()
    f.forest(f.R["r2"]["above"], S.rank_from_fe(f.fe_now))


REFUSALS = {"neighbours without free energies": _refusal_nn_without_fe,
            "neighbours after populations that followed free energies": _refusal_nn_after_populations,
            "free energies of an index that is not resident": _refusal_index,
            "free energies after a pair list": _refusal_fe_after_pairs,
            "free energies after a forest": _refusal_fe_after_forest,
            "a rank that is no permutation": _refusal_rank}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusals_are_codes_and_leave_the_session_usable(dens, one, which):
    ref, R, name = one(10)
    f = S.open_flow(dens, ref, f"{name}: refused: {which}", R=R, n_devices=1)
    with f.s:
        REFUSALS[which](f)


# ---- 3. radius counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", sorted(S.ONE_DEVICE))
def test_radius_counts_grow_and_shrink_in_one_session(dens, one, D):
    ref, R, name = one(D)
    f = S.open_flow(dens, ref, f"{name}: radius counts", R=R, n_devices=1)
    with f.s:
        for radii in S.count_lists(R):
            f.pops(radii)
            for k in sorted({0, len(radii) // 2, len(radii) - 1}):
                f.fe(k)
            f.nn()        # (under the free energies of the last index)


# ---- 4. optional outputs ----------------------------------------------------------------------------------------------------
def test_optional_outputs(dens, one):
    ref, R, name = one(24)
    f = S.open_flow(dens, ref, f"{name}: optional outputs", R=R, n_devices=1)
    with f.s:
        f.pops(R["multi3"], fetch=False)
        f.fe(1, fetch=False)                 # (max_pop is returned and checked by Flow.fe)
        f.nn()                               # all outputs: the values every partial fetch below is held to as well
        names = ("nn_idx", "nn_d2", "hd_idx", "hd_d2", "sigma2")
        for keep in names:
            f.nn(step=f"{keep} alone", **{k: k == keep for k in names})
        f.nn(step="sigma2 and nn_d2", nn_idx=False, hd_idx=False, hd_d2=False)
        f.nn(step="no output at all", **{k: False for k in names})
        # the resident values, through the caller's rank: a forest over what stayed on the device
        f.forest(R["r2"]["above"], S.rank_from_fe(f.fe_now))
        f.nn(step="after the forest")


def test_sigma2_is_a_double_sum(dens, probe, oracle):
    """nn_d2 that a float accumulator cannot add up (sessionref.sigma_data): sigma2 with nn_d2 fetched, and alone --
    through the temporary copy of nn_d2"""
    ref = S.Ref(probe, oracle, S.sigma_data())
    f = S.open_flow(dens, ref, "sigma2 beyond a float sum", R=S.radii_of(ref), n_devices=1)
    with f.s:
        f.pops([1.0, 2.0])
        f.fe(1)
        want, s2 = f.nn()
        assert S.float_sum_differs(want[1])
        f.nn(step="sigma2 alone", nn_idx=False, nn_d2=False, hd_idx=False, hd_d2=False)


# ---- 5. several "devices" on the one GPU ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.MULTI, ids=S.multi_id)
def test_sessions_of_several_devices(dens, probe, oracle, monkeypatch, case):
    n, D, G, merge, poison = case
    monkeypatch.setenv("DC_SESSION_ALLOW_DUPLICATE_DEVICES", "1")
    monkeypatch.setenv("DC_SESSION_NN_MERGE", merge)
    monkeypatch.delenv("DC_SESSION_DEVICES", raising=False)
    monkeypatch.delenv("DC_SESSION_MERGE", raising=False)
    monkeypatch.delenv("DC_SESSION_FORCE_RCCL", raising=False)
    c, clean = S.multi_data(case)
    ref = S.Ref(probe, oracle, c)
    R = S.radii_of(ref if poison is None else S.Ref(probe, oracle, clean))
    assert ref.flagged == (poison is not None)
    f = S.open_flow(dens, ref, "devices " + S.multi_id(case), R=R, devices=[0] * G)
    with f.s:
        assert f.s.n_devices == G and f.s.merge_mode == 2 and not f.s.uses_rccl
        assert "THROUGH THE HOST" in f.s.merge_note and "more than once" in f.s.merge_note, f.s.merge_note
        f.reduced()
    log(S.multi_id(case), "block rows", dens.neighbor_block_rows(n, D, G))


# ---- 6. two sessions at once ------------------------------------------------------------------------------------------------
def test_two_sessions_and_call_by_call_sweeps_interleaved(dens, one):
    import torch
    from crossref import gpu, same_nn
    ref_a, R_a, name_a = one(10)
    ref_b, R_b, name_b = one(24)
    a = S.open_flow(dens, ref_a, f"{name_a}: first of two", R=R_a, n_devices=1)
    b = S.open_flow(dens, ref_b, f"{name_b}: second of two", R=R_b, n_devices=1)
    ct = gpu(ref_b.c)       # call-by-call sweeps of density: their own workspace, on the second session's data
    with a.s:
        with b.s:
            a.pops(R_a["multi9"])
            b.pops(R_b["multi3"], fetch=False)
            got = dens.calculate_populations_partial(ct, R_b["multi3"])
            S.same_ints(got.cpu().numpy(), ref_b.pops(R_b["multi3"]), "call-by-call populations between session calls")
            a.fe(4)
            b.fe(1)
            a.nn()
            fe = ref_b.fe(ref_b.pops(R_b["one"])[0])
            same_nn(dens.nearest_neighbors_partial(ct, gpu(fe)), ref_b.nn(fe), "call-by-call neighbours between session calls")
            b.nn()
            a.forest(R_a["r2"]["above"], S.rank_from_fe(a.fe_now))
            b.pairs(R_b["r2"]["at"])
            a.nn()
            b.nn()
        # the second session is closed: the first must still answer, from what it holds
        a.nn()
        a.pops(R_a["multi3"])
        a.fe(2)
        a.nn()
        torch.cuda.synchronize()


# ---- 7. dc_hip_density_all --------------------------------------------------------------------------------------------------
def density_all(c, radii, fe_index, n_devices, fe=True, nn=("nn_idx", "nn_d2", "hd_idx", "hd_d2"), pops=True):
    """-> (status, message, dict of the outputs that were asked for)"""
    from clustering_amd import capi
    n, d = c.shape
    rad = np.ascontiguousarray(radii, dtype=np.float32)
    out = {"pops": np.full((rad.size, n), 0xABCD, dtype=np.uint32), "fe": np.full(n, -7.0, dtype=np.float32)}
    for k in ("nn_idx", "hd_idx"):
        out[k] = np.full(n, 0xABCD, dtype=np.uint32)
    for k in ("nn_d2", "hd_d2"):
        out[k] = np.full(n, -7.0, dtype=np.float32)
    use = {"pops": pops, "fe": fe, **{k: k in nn for k in ("nn_idx", "nn_d2", "hd_idx", "hd_d2")}}
    p = lambda k: out[k].ctypes.data_as(C.c_void_p) if use[k] else None
    rc = capi.lib.dc_hip_density_all(c.ctypes.data_as(C.c_void_p), n, d, rad.ctypes.data_as(C.c_void_p), rad.size, fe_index,
                                     n_devices, p("pops"), p("fe"), p("nn_idx"), p("nn_d2"), p("hd_idx"), p("hd_d2"))
    if rc == capi.DC_ERR_HIP:
        pytest.exit("dc_hip_density_all returned DC_ERR_HIP: " + capi.lib.dc_hip_last_error().decode("utf-8", "replace"), returncode=3)
    return rc, capi.lib.dc_hip_last_error().decode("utf-8", "replace"), {k: v for k, v in out.items() if use[k]}


def check_density_all(ref, radii, fe_index, got):
    want_p = ref.pops(radii)
    S.same_ints(got["pops"], want_p, ("density_all pops", fe_index))
    want_fe = ref.fe(want_p[fe_index])
    if "fe" in got:
        S.same_floats(got["fe"], want_fe, ("density_all fe", fe_index))
    if "nn_idx" in got:
        want = ref.nn(want_fe)
        for k, name in enumerate(("nn_idx", "nn_d2", "hd_idx", "hd_d2")):
            (S.same_ints if k % 2 == 0 else S.same_floats)(got[name], want[k], ("density_all", name, fe_index))


@pytest.mark.parametrize("n_devices", [0, 1])
def test_density_all_every_free_energy_index(dens, one, n_devices):
    from clustering_amd import capi
    ref, R, name = one(10)
    radii = R["multi3"]
    for fe_index in range(len(radii)):
        rc, msg, got = density_all(ref.c, radii, fe_index, n_devices)
        assert rc == capi.DC_OK, msg
        check_density_all(ref, radii, fe_index, got)


def test_density_all_optional_and_refused_arguments(dens, one, probe, oracle):
    from clustering_amd import capi
    ref, R, name = one(10)
    radii = R["multi9"]
    # neighbours skipped, with and without the free energies
    for fe in (True, False):
        rc, msg, got = density_all(ref.c, radii, 4, 1, fe=fe, nn=())
        assert rc == capi.DC_OK, msg
        check_density_all(ref, radii, 4, got)
    # refused: incomplete neighbour outputs (each one missing by turns, and the free energies), an index out of range,
    # no populations, no radii
    full = ("nn_idx", "nn_d2", "hd_idx", "hd_d2")
    for missing in full[1:]:
        rc, msg, got = density_all(ref.c, radii, 0, 1, nn=tuple(k for k in full if k != missing))
        assert rc == capi.DC_ERR_INVALID_ARGUMENT and msg.strip(), (missing, rc, msg)
    rc, msg, got = density_all(ref.c, radii, 0, 1, fe=False)
    assert rc == capi.DC_ERR_INVALID_ARGUMENT and msg.strip(), (rc, msg)
    for bad in (len(radii), len(radii) + 5, 2 ** 40):
        rc, msg, got = density_all(ref.c, radii, bad, 1)
        assert rc == capi.DC_ERR_INVALID_ARGUMENT and msg.strip(), (bad, rc, msg)
    rc, msg, got = density_all(ref.c, radii, 0, 1, pops=False)
    assert rc == capi.DC_ERR_INVALID_ARGUMENT and msg.strip(), (rc, msg)
    rc, msg, got = density_all(ref.c, [], 0, 1)
    assert rc == capi.DC_ERR_INVALID_ARGUMENT and msg.strip(), (rc, msg)
    # ... and the next valid call is answered
    rc, msg, got = density_all(ref.c, radii, 8, 1)
    assert rc == capi.DC_OK, msg
    check_density_all(ref, radii, 8, got)
    # one and two rows
    for n in (1, 2):
        for D in (3, 24, 70):
            small = S.Ref(probe, oracle, S.data("lattice", n, D, 300 + n))
            rad = S.radii_of(small)["multi9"]
            for n_devices in (0, 1):
                rc, msg, got = density_all(small.c, rad, 3, n_devices)
                assert rc == capi.DC_OK, msg
                check_density_all(small, rad, 3, got)


# ---- 8. a one-rank RCCL communicator, in ONE child process ------------------------------------------------------------------
RCCL_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import density as dens     # (torch and its RCCL first: a process that loads libdcdensity.so before
from clustering_amd import capi                 #  torch binds another copy of the HIP runtime, and ncclCommInitAll finds no device)
from oracle.oracle import Oracle, Probe
import sessionref as S
probe, oracle = Probe(capi.CANON_ORDER), Oracle()
name, kind, n, d, seed = S.ONE_DEVICE[10]
ref = S.Ref(probe, oracle, S.data(kind, n, d, seed))
R = S.radii_of(ref)
modes = []
for merge in ("allgather", "allreduce"):
    os.environ["DC_SESSION_NN_MERGE"] = merge          # (read by every neighbour call)
    f = S.open_flow(dens, ref, "one-rank communicator, " + merge, R=R, n_devices=1)
    with f.s:
        modes.append((f.s.merge_mode, f.s.uses_rccl, f.s.merge_note))
        f.reduced()
print("SESSION-EDGES", modes)
"""


def test_reduced_programme_over_a_one_rank_communicator():
    """DC_SESSION_FORCE_RCCL=1: the collectives' call path (grouped all-reduce of the populations and the forest's
    candidates, all-gather of the neighbour blocks / all-reduce(min) of the packed words) on the lattice with ties.  Whether
    RCCL comes up on this machine is test_gpu_session.test_session_over_rccl's to say: the programme here must give the
    referee's values in whichever mode the session reports."""
    env = dict(os.environ, DC_SESSION_FORCE_RCCL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("DC_SESSION_MERGE", "DC_SESSION_DEVICES", "DC_SESSION_ALLOW_DUPLICATE_DEVICES"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", RCCL_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=env)
    # the child died on the GPU or met a HIP error: nothing more is started on the device
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or S.HIP_ERROR_MARK in r.stderr:
        pytest.exit(f"the one-rank RCCL child ended with status {r.returncode}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("SESSION-EDGES")]
    assert lines, (r.stdout[-500:], r.stderr[-1500:])
    log(lines[-1])
