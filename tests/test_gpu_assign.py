"""The assigner on the device (dc_hip_assign_*, dc_hip_assigner_*; density.Reference.assign_device, density.Assigner;
DESIGN.md 4.30): every value bit for bit against the path it replaces -- Reference.assign, assign_frames,
assign_frames_wide_pruned -- and the one property the batch call adds: it returns with its work still queued.
Cases and premises: tests/assignref.py, tests/test_assign_cases.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import assignref as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("states", "pops", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2")
INVALID, WORKSPACE = -1, -5


@pytest.fixture(scope="module")
def dens():
    from clustering_amd import density
    return density


@pytest.fixture(scope="module")
def capi():
    from clustering_amd import capi
    return capi


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    """bit for bit: integers as they are, floats by their bits"""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def reference(D, n=cases.N_REF):
    R = cases.reference(D, n)
    return R, gpu(R)


def open_(dens, Rt, max_batch, radius, states, **kw):
    D = Rt.shape[1]
    if D <= 64:
        return dens.NarrowReference(Rt, max_batch, radius=radius, ref_states=states, **kw)
    return dens.Reference(Rt, max_batch, radius=radius, ref_states=states)


def check(h, Q, what=""):
    """assign_device against assign on every key of the dict -> (assign's dict, info after assign_device)"""
    q = gpu(Q)
    want = h.assign(q)
    got = h.assign_device(q)
    info = h.info()
    assert set(got) == set(want)
    for key in want:
        if key == "max_pop":
            assert got[key] == want[key]
        else:
            assert got[key].dtype == want[key].dtype and same(got[key], want[key]), (what, key)
    return want, info


@pytest.mark.parametrize("D", cases.NARROW + cases.WIDE)
def test_assign_device_equals_assign_batch_after_batch(dens, D):
    R, Rt = reference(D)
    states = cases.states_of(len(R))
    with open_(dens, Rt, cases.MAX_BATCH, cases.radius(D), states) as h:
        for k, n_q in enumerate(cases.BATCHES):
            want, info = check(h, cases.batch(R, n_q, seed=40 + k), (D, n_q))
            assert info[3] == 0 and info[0] > 0, ("a clean batch runs on the matrix cores", D, n_q, info)
            assert int(want["pops"].max()) > 0 and (n_q == 1 or len(torch.unique(want["states"])) > 1), "the case says something"
        assert h.info()[4] == 1, "the reference was prepared once"
        assert h.assign_device(gpu(R[:0]))["states"].shape == (0,)


def test_the_lattice_gives_every_free_energy(dens):
    Q, R = cases.lattice()
    states = cases.states_of(len(R))
    for max_pop in (None, cases.LATTICE_LOW_MAX_POP):
        with dens.NarrowReference(gpu(R), 512, radius=cases.LATTICE_R, ref_states=states) as h:
            assert h.max_pop == 1401
            if max_pop is not None:
                h.max_pop = max_pop   # (the scale is the caller's: dc_hip_assign_open_dev takes it as an argument)
            want, info = check(h, Q, ("lattice", max_pop))
            got = h.assign_device(gpu(Q))
            assert info[3] == 0
        pops = got["pops"].cpu().numpy()
        assert (pops == cases.lattice_populations(Q, R)).all() and set(range(1401)) <= set(pops.tolist())
        fe = got["fe"]
        assert same(fe, dens.calculate_free_energies_against(got["pops"].contiguous(), h.max_pop))
        fe = fe.cpu().numpy()
        assert np.isposinf(fe[pops == 0]).all() and (pops == 0).sum() == 1
        assert (fe[pops > h.max_pop] < 0).all() and (fe[(pops > 0) & (pops < h.max_pop)] > 0).all()
        assert (pops > h.max_pop).sum() == (0 if max_pop is None else 401)


@pytest.mark.parametrize("D", [10, 100])
def test_queries_beyond_every_blob(dens, D):
    R, Rt = reference(D)
    Q = cases.far_batch(R, 300)
    rows = cases.ref.headroom_rows(300)
    with open_(dens, Rt, 300, cases.radius(D), cases.states_of(len(R))) as h:
        want, info = check(h, Q, "far")
        assert info[3] == 0 and info[0] > 0, "inside the 4 x extent: the matrix cores answer"
    assert (want["pops"][rows] == 0).all() and torch.isposinf(want["fe"][rows]).all()
    # every reference row has a lower free energy than +inf: the nearest row is the nearest lower one, and gives the state
    assert torch.equal(want["hd_idx"][rows], want["nn_idx"][rows]) and (want["nn_idx"][rows] < len(R)).all()
    assert torch.equal(want["states"][rows].cpu(), torch.from_numpy(cases.states_of(len(R)))[want["nn_idx"][rows].cpu().long()])


@pytest.mark.parametrize("D", [3, 100])
def test_small_references(dens, D):
    full = reference(D)[0]
    one = full[:1]
    with open_(dens, gpu(one), 8, cases.radius(D), np.array([7], np.int32)) as h:
        want, _ = check(h, np.concatenate([np.repeat(one, 5, axis=0), full[1:3]]), "reference of 1 row")
        assert h.max_pop == 1 and (want["states"] == 7).all() and (want["pops"][:5] == 1).all() and (want["nn_idx"] == 0).all()
    R33 = full[:33]
    with open_(dens, gpu(R33), 64, cases.radius(D), cases.states_of(33)) as h:
        check(h, cases.batch(R33, 50), "reference of 33 rows")
        check(h, R33[::-1].copy(), "the reference itself, reversed")


def test_ties_and_equal_free_energies(dens):
    Q, R, states = cases.tie_case()
    a, b = cases.TIE_ROWS
    with dens.NarrowReference(gpu(R), 8, radius=cases.TIE_RADIUS, ref_states=states) as h:
        want, _ = check(h, Q, "ties")
        assert h.max_pop == 8
    none = len(R) + 1
    assert (want["pops"] == 8).all() and (want["fe"] == 0).all(), "the queries' free energy equals the duplicates'"
    assert (want["hd_idx"] == none).all(), "equal is not lower: hd is none"
    assert (want["nn_idx"] == a).all(), "of the tied rows the lowest"
    assert (want["states"] == int(states[a])).all() and states[a] != states[b], "the state comes through nn, from the lower row"


@pytest.mark.parametrize("D", [10, 100])
def test_a_flagged_batch_and_the_clean_one_after_it(dens, D):
    R, Rt = reference(D)
    with open_(dens, Rt, 300, cases.radius(D), cases.states_of(len(R))) as h:
        _, info = check(h, cases.flagged_batch(R, 300), "flagged")
        assert info[:4] == (0, 0, 0, 2), info
        _, info = check(h, cases.batch(R, 300, seed=5), "clean again")
        assert info[3] == 0 and info[0] > 0, info


def test_outputs_left_null_through_the_c_call(dens, capi):
    R, Rt = reference(10)
    q = gpu(cases.batch(R, 300))
    with open_(dens, Rt, 300, cases.radius(10), cases.states_of(len(R))) as h:
        want = h.assign_device(q)
        a = h._assigner()
        for keep in ((), ("fe",), ("pops", "hd_idx"), ("nn_idx", "nn_d2", "hd_d2")):
            out = {k: torch.full((300,), -7, dtype=want[k].dtype, device="cuda") for k in ("states",) + keep}
            args = [C.c_void_p(out[k].data_ptr()) if k in out else None for k in KEYS]
            rc = capi.lib.dc_hip_assign_batch_dev(a, C.c_void_p(q.data_ptr()), 300, *args,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, capi.lib.dc_hip_last_error()
            for k in out:
                assert same(out[k], want[k]), (keep, k)
        # zero rows: DC_OK, nothing written, whatever the pointers
        assert capi.lib.dc_hip_assign_batch_dev(a, None, 0, None, None, None, None, None, None, None, None) == 0


def test_refusals(dens, capi):
    lib = capi.lib
    R, Rt = reference(10)
    r = cases.radius(10)
    states = gpu(cases.states_of(len(R)))
    need = lib.dc_hip_assign_workspace_bytes(len(R), 200)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    dev = lambda t: C.c_void_p(t.data_ptr())
    h = C.c_void_p(0x1)

    def refused(handle, code, *args):
        h.value = 0x1
        assert lib.dc_hip_assign_open_dev(handle._h, *args, None, C.byref(h)) == code and not h.value, args
        assert "dc_hip_assign_open_dev" in lib.dc_hip_last_error().decode()

    with dens.NarrowReference(Rt, 200, max_radius=r) as bare:
        refused(bare, INVALID, dev(states), 100, r, dev(ws), need)   # before set_free_energies
        assert "free energies" in lib.dc_hip_last_error().decode()
    with dens.NarrowReference(Rt, 200, radius=r, ref_states=cases.states_of(len(R))) as ref:
        above = float(np.nextafter(np.float32(r), np.float32(np.inf))) * 1.001
        refused(ref, INVALID, dev(states), 100, above, dev(ws), need)          # a radius above max_radius
        refused(ref, INVALID, dev(states), 0, r, dev(ws), need)                # max_pop == 0
        refused(ref, INVALID, dev(states), 100, float("nan"), dev(ws), need)
        refused(ref, INVALID, dev(states), 100, -1.0, dev(ws), need)
        refused(ref, INVALID, None, 100, r, dev(ws), need)
        refused(ref, WORKSPACE, dev(states), 100, r, dev(ws), need - 1)        # a short workspace
        refused(ref, WORKSPACE, dev(states), 100, r, None, need)
        q = gpu(cases.batch(R, 201))
        a = ref._assigner()
        out = torch.zeros(201, dtype=torch.int32, device="cuda")
        rc = lib.dc_hip_assign_batch_dev(a, dev(q), 201, dev(out), None, None, None, None, None, None, None)
        assert rc == INVALID and "dc_hip_assign_batch_dev" in lib.dc_hip_last_error().decode(), "n_query > max_batch"
        assert lib.dc_hip_assign_batch_dev(a, dev(q), 200, None, None, None, None, None, None, None, None) == INVALID, "d_states is required"
        assert ref.assign_device(q)["states"].shape == (201,), "the Python call chunks"
    with pytest.raises(ValueError):
        with dens.NarrowReference(Rt, 200, max_radius=r) as bare:
            bare.assign_device(gpu(cases.batch(R, 10)))
    with dens.Reference(reference(100)[1], 200) as bare:
        h.value = 0x1
        assert lib.dc_hip_assign_open_wide_dev(bare._h, dev(states), 100, r, dev(ws), need, None, C.byref(h)) == INVALID and not h.value
        assert "dc_hip_assign_open_wide_dev" in lib.dc_hip_last_error().decode()


CHILD_STREAM = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import density as dens
import assignref as cases
D = int(sys.argv[2])
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
R = cases.reference(D)
q = gpu(cases.batch(R, 300))
cls = dens.NarrowReference if D <= 64 else dens.Reference
h = cls(gpu(R), 300, radius=cases.radius(D), ref_states=cases.states_of(len(R)))
torch.cuda.synchronize()
side = torch.cuda.Stream()
with h, torch.cuda.stream(side):
    want = h.assign(q)
    h.assign_device(q)   # (builds the assigner: its table and workspace)
    side.synchronize()

    def blocker_ms(cycles):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        torch.cuda._sleep(cycles)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    cycles, ms = 1_000_000, 0.0   # (whatever the clock behind the cycles: size the blocker from what is measured)
    for _ in range(5):
        ms = blocker_ms(cycles)
        if ms >= 80.0:
            break
        cycles = int(cycles * min(100.0 / max(ms, 1e-3), 50.0))
    print(f"blocker: {cycles} cycles, {ms:.1f} ms")
    assert 50.0 <= ms < 5000.0, ms

    def probe(call):
        torch.cuda._sleep(cycles)
        front = torch.cuda.Event()
        front.record()
        out = call(q)
        pending = not front.query()
        side.synchronize()
        return out, pending

    got, pending = probe(h.assign_device)
    assert pending, "assign_device synchronised with the host"
    for key in ("states", "pops", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2"):
        assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), key
    _, pending = probe(h.assign)
    assert not pending, "Reference.assign goes through the host: what the batch call removes"
torch.cuda.synchronize()
print("ok: queued")
"""


@pytest.mark.timeout(120)
@pytest.mark.parametrize("D", [10, 100])
def test_assign_device_returns_with_its_work_queued(D):
    """The stream-order promise: behind a blocker of at least 50 ms on a side stream, assign_device returns while the
    event recorded in front of it is still pending; Reference.assign, which hands its free energies through the host,
    returns only after it.  In a process of its own: the side stream and the blocker stay out of the suite's process."""
    r = subprocess.run([sys.executable, "-c", CHILD_STREAM, ROOT, str(D)], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0 and "ok: queued" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout.strip().splitlines()[0])


CHILD_HOST = r"""
import hashlib, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import density as dens
import assignref as cases
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
digest = hashlib.sha256()
for D, path in ((10, 0), (100, 1), (300, 2)):
    R = cases.reference(D)
    Q = np.concatenate([cases.batch(R, 2200, seed=81), cases.far_batch(R, 300, seed=82)])
    states, r = cases.states_of(len(R)), cases.radius(D)
    with dens.Assigner(R, states, r, 700) as a:
        assert a.path == path, (D, a.path)
        got = a.assign(Q)          # four chunks: 700, 700, 700, 400
        again = a.assign(Q[:701])  # the slots are taken again
        pops_ref, fe_ref, max_pop = a.reference()
    frames = dens.assign_frames_wide_pruned if 65 <= D <= 256 else dens.assign_frames
    want = {k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in frames(gpu(Q), gpu(R), r, states).items()}
    for key in ("states", "pops", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2"):
        assert got[key].dtype.itemsize == 4 and got[key].tobytes() == want[key].tobytes(), (D, key)
        assert again[key].tobytes() == want[key][:701].tobytes(), (D, key, "second call")
        digest.update(got[key].tobytes())
    assert pops_ref.tobytes() == want["pops_ref"].tobytes() and fe_ref.tobytes() == want["fe_ref"].tobytes()
    assert max_pop == want["max_pop"] == int(pops_ref.max())
print("ok:", digest.hexdigest())
"""

CHILD_CANON = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
import assignref as cases
assert capi.lib.dc_hip_canon_order().decode() == sys.argv[2]
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
for D in (10, 100):
    R = cases.reference(D)
    q = gpu(cases.far_batch(R, 700))
    cls = dens.NarrowReference if D <= 64 else dens.Reference
    with cls(gpu(R), 300, radius=cases.radius(D), ref_states=cases.states_of(len(R))) as h:
        want, got = h.assign(q), h.assign_device(q)
        assert h.info()[3] == 0 and h.info()[0] > 0
    for key in ("states", "pops", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2", "pops_ref", "fe_ref"):
        assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), (D, key)
print("ok:", sys.argv[2])
"""


def child(script, *args, **env):
    r = subprocess.run([sys.executable, "-c", script, ROOT, *args], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ok:" in r.stdout
    return r.stdout.split("ok:")[1].split()[0]


def test_the_host_assigner_with_and_without_overlap():
    env = {k: v for k, v in os.environ.items() if k != "DC_ASSIGN_OVERLAP"}
    r = subprocess.run([sys.executable, "-c", CHILD_HOST, ROOT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ok:" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    default = r.stdout.split("ok:")[1].split()[0]
    assert child(CHILD_HOST, DC_ASSIGN_OVERLAP="0") == default, "one stream or two: the same outputs"


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_the_other_summation_orders(order):
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    assert child(CHILD_CANON, order, DC_CANON_ORDER=order) == order
