"""The host assigner on the resident reference of 257..1024 columns (dc_hip_assigner_open_flags with
DC_ASSIGNER_XWIDE_REFERENCE, DC_ASSIGN_XWIDE=1; density.Assigner(xwide=True)): path 3, every array
byte-equal to density.assign_frames (the direct kernels) and to path 2's output; outside those widths the flag changes
nothing; dc_hip_assign_batch_dev on an XWideReference equals its assign.  In child processes, as tests/test_gpu_assign.py
runs the host assigner.  Cases: tests/assignref.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD_HOST = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import density as dens
import assignref as cases
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
KEYS = ("states", "pops", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2")
D, flag, want_path, want_plain_path = int(sys.argv[2]), sys.argv[3] == "flag", int(sys.argv[4]), int(sys.argv[5])
R = cases.reference(D)
Q = np.concatenate([cases.batch(R, 2200, seed=81), cases.far_batch(R, 300, seed=82)])
states, r = cases.states_of(len(R)), cases.radius(D)
with dens.Assigner(R, states, r, 700, xwide=flag) as a:
    assert a.path == want_path, (D, a.path)
    got = a.assign(Q)          # four chunks: 700, 700, 700, 400
    again = a.assign(Q[:701])  # the slots are taken again
    pops_ref, fe_ref, max_pop = a.reference()
if want_path == 3:
    # path 2 from an Assigner without the flag -- unless the environment selects path 3 for it too
    with dens.Assigner(R, states, r, 700) as b:
        assert b.path == want_plain_path, b.path
        plain = b.assign(Q)
        plain_ref = b.reference()
    for key in KEYS:
        assert got[key].tobytes() == plain[key].tobytes(), (D, key, "path 2")
    assert pops_ref.tobytes() == plain_ref[0].tobytes() and fe_ref.tobytes() == plain_ref[1].tobytes() and max_pop == plain_ref[2]
    want = {k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in dens.assign_frames(gpu(Q), gpu(R), r, states, variant="direct").items()}
    for key in KEYS:
        assert got[key].dtype.itemsize == 4 and got[key].tobytes() == want[key].tobytes(), (D, key)
        assert again[key].tobytes() == want[key][:701].tobytes(), (D, key, "second call")
    assert pops_ref.tobytes() == want["pops_ref"].tobytes() and fe_ref.tobytes() == want["fe_ref"].tobytes()
    assert max_pop == want["max_pop"] == int(pops_ref.max())
    assert int(want["pops"].max()) > 0 and len(np.unique(want["states"])) > 1, "the case says something"
print("ok:", want_path)
"""

CHILD_DEVICE = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import density as dens
import assignref as cases
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
D = int(sys.argv[2])
R = cases.reference(D)
q = gpu(np.concatenate([cases.batch(R, 500, seed=81), cases.far_batch(R, 200, seed=82)]))
with dens.XWideReference(gpu(R), 300, radius=cases.radius(D), ref_states=cases.states_of(len(R))) as h:
    want, got = h.assign(q), h.assign_device(q)   # (three chunks: 300, 300, 100)
    assert h.info()[3] == 0 and h.info()[0] > 0
for key in ("states", "pops", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2", "pops_ref", "fe_ref"):
    assert torch.equal(got[key].view(torch.int32), want[key].view(torch.int32)), (D, key)
assert got["max_pop"] == want["max_pop"]
print("ok:", D)
"""


def child(script, *args, **env):
    base = {k: v for k, v in os.environ.items() if k != "DC_ASSIGN_XWIDE"}
    r = subprocess.run([sys.executable, "-c", script, ROOT, *args], capture_output=True, text=True, timeout=600, env=dict(base, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ok:" in r.stdout
    return r.stdout.split("ok:")[1].split()[0]


@pytest.mark.parametrize("D", [300, 1024])
def test_the_flag_selects_path_3_and_every_array_equals_the_direct_kernels_and_path_2(D):
    assert child(CHILD_HOST, str(D), "flag", "3", "2") == "3"


@pytest.mark.parametrize("D,path", [(10, 0), (100, 1)])
def test_outside_these_widths_the_flag_changes_nothing(D, path):
    assert child(CHILD_HOST, str(D), "flag", str(path), str(path)) == str(path)


def test_the_environment_selects_path_3_without_the_flag():
    assert child(CHILD_HOST, "300", "noflag", "3", "3", DC_ASSIGN_XWIDE="1") == "3"
    assert child(CHILD_HOST, "300", "noflag", "2", "2", DC_ASSIGN_XWIDE="0") == "2", "only the value 1 opts in"


def test_the_batch_call_on_an_xwide_reference_equals_its_assign():
    assert child(CHILD_DEVICE, "300") == "300"
