"""GPU: resident sessions on the pruned wide matrix-core sweeps (density.Session(..., wide=True), 65..256 columns) held to
the referee of tests/sessionref.py -- the probe's canonical d2 matrix, the oracle's free energies and sigma2, the contract
of a forest -- through the same runner, with the wide sessions' rule for who answered (tests/widesessionref.py: evaluated
tile pairs > 0 on unflagged data, 0 on flagged data and under a NaN free energy).  One device; 2, 3 and 5 "devices" on the
one GPU with both neighbour merges; 0 rows; the flag outside 65..256 columns; a default session of wide rows, which stays on
the direct kernels; DC_SESSION_WIDE=1; and a one-rank RCCL communicator in one fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sessionref as S
import widesessionref as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SESSION_ENV = ("DC_SESSION_WIDE", "DC_SESSION_DEVICES", "DC_SESSION_MERGE", "DC_SESSION_FORCE_RCCL", "DC_SESSION_NN_MERGE",
               "DC_SESSION_ALLOW_DUPLICATE_DEVICES")


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


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for k in SESSION_ENV:
        monkeypatch.delenv(k, raising=False)


# the whole flow of a run: populations of 3, 9 and 1 radii, free energies, handed-in free energies, neighbours + sigma2, the
# pair list and the forest, with every hand-over between two sweeps of different kinds
PROGRAMME = [("pops", "multi3", True), ("fe", 1, True), ("nn",), ("forest", "above", "fe"), ("pops", "multi9", True),
             ("fe", "last", True), ("nn",), ("pairs", "above"), ("pops", "one", False), ("fe", 0, True), ("nn",), ("nn",),
             ("setfe", "ties_ulp"), ("nn",), ("forest", "at", "random"), ("setfe", "nan"), ("nn",), ("pairs", "at")]


@pytest.mark.parametrize("case", W.ONE_DEVICE, ids=lambda c: f"n{c[0]}-D{c[1]}")
def test_one_device(dens, probe, oracle, case):
    ref = S.Ref(probe, oracle, W.one_data(case))
    f = W.open_wide_flow(dens, ref, f"wide session {case}", R=S.radii_of(ref), n_devices=1)
    with f.s:
        assert f.s.wide and f.s.n_devices == 1 and f.s.merge_mode == 0
        f.run(PROGRAMME)


@pytest.mark.parametrize("case", W.MULTI, ids=S.multi_id)
def test_several_devices(dens, probe, oracle, monkeypatch, case):
    n, D, G, merge, poison = case
    monkeypatch.setenv("DC_SESSION_ALLOW_DUPLICATE_DEVICES", "1")
    monkeypatch.setenv("DC_SESSION_NN_MERGE", merge)
    ref, R = W.multi_ref(probe, oracle, case)      # (flagged by the wide sweeps' rule: 6e16 is not)
    assert ref.flagged == (poison in ("nan", "inf", "2e18"))
    f = W.open_wide_flow(dens, ref, "wide devices " + S.multi_id(case), R=R, devices=[0] * G)
    with f.s:
        assert f.s.wide and f.s.n_devices == G and f.s.merge_mode == 2 and not f.s.uses_rccl
        f.reduced()
        if n and not ref.flagged:
            # who answered, once more by hand: populations and neighbours on the matrix cores of every device with a block
            f.pops(R["one"])
            f.fe(0)
            f.nn()
            pop_tiles, nn_tiles = f.s.counters()
            assert pop_tiles > 0 and nn_tiles > 0, (pop_tiles, nn_tiles)


def test_no_rows(dens, probe, oracle):
    ref = S.Ref(probe, oracle, S.data("lattice", 0, 100, 1))
    f = W.open_wide_flow(dens, ref, "wide session of no rows", R=S.radii_of(ref), n_devices=1)
    with f.s:
        assert f.s.wide
        f.run([("pops", "multi3", True), ("nn",), ("pairs", "at"), ("forest", "at", "identity")])
        assert f.s.counters() == (0, 0)
        f.call(f.s.set_free_energies, np.zeros(0, dtype=np.float32))


@pytest.mark.parametrize("case", W.NARROW_AND_BEYOND, ids=lambda c: f"n{c[0]}-D{c[1]}")
def test_the_flag_changes_nothing_outside_the_wide_columns(dens, probe, oracle, case):
    n, D, seed = case
    ref = S.Ref(probe, oracle, S.data("lattice", n, D, seed))
    f = W.open_wide_flow(dens, ref, f"flag at D={D}", R=S.radii_of(ref), n_devices=1)
    with f.s:
        assert not f.s.wide
        f.run(PROGRAMME)      # (who answered: the rule of a default session, sessionref.Flow.who)


def test_a_default_session_of_wide_rows_stays_on_the_direct_kernels(dens, probe, oracle):
    n, D, seed = W.DEFAULT_CASE
    ref = S.Ref(probe, oracle, S.data("lattice", n, D, seed))
    f = S.open_flow(dens, ref, "default session at D=100", R=S.radii_of(ref), n_devices=1)
    with f.s:
        assert not f.s.wide
        f.run(PROGRAMME[:7])      # (sessionref.Flow.who: 0 tiles at every step)
        assert f.s.counters() == (0, 0)


def test_the_environment_sets_the_flag(dens, probe, oracle, monkeypatch):
    """DC_SESSION_WIDE=1: dc_hip_session_open, and so dc_hip_density_all, run the wide sweeps; any other value does not"""
    import ctypes as C
    from clustering_amd import capi
    n, D, seed = W.DEFAULT_CASE
    ref = S.Ref(probe, oracle, S.data("lattice", n, D, seed))
    R = S.radii_of(ref)
    monkeypatch.setenv("DC_SESSION_WIDE", "0")
    with dens.Session(ref.c, n_devices=1) as s:
        assert not s.wide
    monkeypatch.setenv("DC_SESSION_WIDE", "1")
    f = W.WideFlow(dens, ref, dens.Session(ref.c, n_devices=1), "DC_SESSION_WIDE=1", R=R)
    with f.s:
        assert f.s.wide
        f.run(PROGRAMME[:3])
    radii = np.array(R["multi3"], dtype=np.float32)
    n = ref.n
    pops = np.zeros((3, n), dtype=np.uint32)
    fe, nn_d2, hd_d2 = (np.zeros(n, dtype=np.float32) for _ in range(3))
    nn_idx, hd_idx = (np.zeros(n, dtype=np.uint32) for _ in range(2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    capi.check(capi.lib.dc_hip_density_all(p(ref.c), n, ref.D, p(radii), 3, 1, 1, p(pops), p(fe), p(nn_idx), p(nn_d2), p(hd_idx),
                                           p(hd_d2)), "dc_hip_density_all")
    want_p = ref.pops(R["multi3"])
    want_fe = ref.fe(want_p[1])
    want = ref.nn(want_fe)
    S.same_ints(pops, want_p, "density_all pops")
    S.same_floats(fe, want_fe, "density_all fe")
    for k, got in enumerate((nn_idx, nn_d2, hd_idx, hd_d2)):
        (S.same_ints if k % 2 == 0 else S.same_floats)(got, want[k], ("density_all", k))


RCCL_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from clustering_amd import density as dens     # (torch and its RCCL first, as in tests/test_gpu_session_edges.py)
from clustering_amd import capi
from oracle.oracle import Oracle, Probe
import sessionref as S
import widesessionref as W
probe, oracle = Probe(capi.CANON_ORDER), Oracle()
ref = S.Ref(probe, oracle, W.one_data(W.ONE_DEVICE[1]))
R = S.radii_of(ref)
modes = []
for merge in ("allgather", "allreduce"):
    os.environ["DC_SESSION_NN_MERGE"] = merge          # (read by every neighbour call)
    f = W.open_wide_flow(dens, ref, "wide one-rank communicator, " + merge, R=R, n_devices=1)
    with f.s:
        assert f.s.wide
        modes.append((f.s.merge_mode, f.s.uses_rccl, f.s.merge_note))
        f.reduced()
print("WIDE-SESSION", modes)
"""


def test_reduced_programme_over_a_one_rank_communicator():
    """DC_SESSION_FORCE_RCCL=1: the segment forms (segment 0 of 1), the pack, the all-gather and the unpack -- or the word
    pack and the all-reduce(min) -- over a one-rank communicator, in whichever mode the session reports"""
    env = dict(os.environ, DC_SESSION_FORCE_RCCL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("DC_SESSION_MERGE", "DC_SESSION_DEVICES", "DC_SESSION_ALLOW_DUPLICATE_DEVICES", "DC_SESSION_WIDE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", RCCL_CHILD, ROOT], capture_output=True, text=True, timeout=600, env=env)
    # the child died on the GPU or met a HIP error: nothing more is started on the device
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or S.HIP_ERROR_MARK in r.stderr:
        pytest.exit(f"the one-rank RCCL child ended with status {r.returncode}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("WIDE-SESSION")]
    assert lines, (r.stdout[-500:], r.stderr[-1500:])
    print(lines[-1])
