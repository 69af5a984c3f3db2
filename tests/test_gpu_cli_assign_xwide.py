"""GPU: `clustering assign -v` at 300 columns with and without DC_ASSIGN_XWIDE=1 in its environment -- the first run is
served by the resident reference of 257..1024 columns (path 3), the second by the per-call cross sweeps (path 2), and all
four files they write are equal, header lines aside.  Cases: tests/assignref.py."""
import os
import subprocess

import numpy as np
import pytest

import assignref as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "clustering_amd", "bin", "clustering")
D, N_NEW = 300, 700


def data_lines(path):
    return [l for l in open(path).read().splitlines() if l and not l.startswith("#")]


def assign(tmp, radius, tag, env):
    out = {k: str(tmp / f"{k}_{tag}") for k in ("states", "pops", "fe", "nn")}
    r = subprocess.run([CLI, "assign", "-f", str(tmp / "ref.npy"), "-s", str(tmp / "states"), "-q", str(tmp / "new.npy"),
                        "-r", "%.9g" % np.float32(radius), "-o", out["states"], "-p", out["pops"], "-d", out["fe"], "-b", out["nn"],
                        "--batch", "300", "-v"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout, out


def test_the_environment_variable_selects_the_resident_reference_and_the_files_stay_the_same(tmp_path):
    R = cases.reference(D)
    Q = np.concatenate([cases.batch(R, N_NEW - 100, seed=3), cases.far_batch(R, 100, seed=4)])
    np.savetxt(tmp_path / "states", cases.states_of(len(R)), fmt="%d")
    np.save(tmp_path / "ref.npy", R)
    np.save(tmp_path / "new.npy", Q)
    radius = float(np.float32(cases.radius(D)))
    base = {k: v for k, v in os.environ.items() if k != "DC_ASSIGN_XWIDE"}
    said_on, on = assign(tmp_path, radius, "on", dict(base, DC_ASSIGN_XWIDE="1"))
    said_off, off = assign(tmp_path, radius, "off", base)
    assert "served by: the resident reference of 257..1024 columns" in said_on
    assert "served by: the per-call cross sweeps" in said_off
    for k in on:
        lines = data_lines(on[k])
        assert len(lines) == N_NEW and lines == data_lines(off[k]), k
    assert len(set(data_lines(on["states"]))) > 1 and "inf" in data_lines(on["fe"]), "the case says something"
