"""GPU: `clustering assign` against the Python path -- every file it writes, header lines aside, equals what
density.assign_frames / assign_frames_wide_pruned give for the same values in the writers' formats; .npy and ASCII inputs
give identical files; the refusals of the mode.  Cases: tests/assignref.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import assignref as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "clustering_amd", "bin", "clustering")
N_NEW = 700


def data_lines(path):
    return [l for l in open(path).read().splitlines() if l and not l.startswith("#")]


def write_ascii(path, c):
    np.savetxt(path, c, fmt="%.9g")   # (nine digits: the decimal round trip gives the float back)
    assert (np.loadtxt(path, dtype=np.float64, ndmin=2).astype(np.float32) == c).all()


def assign(tmp, ref, new, states, radius, tag, *extra):
    out = {k: str(tmp / f"{k}_{tag}") for k in ("states", "pops", "fe", "nn")}
    r = subprocess.run([CLI, "assign", "-f", str(ref), "-s", str(states), "-q", str(new), "-r", "%.9g" % np.float32(radius),
                        "-o", out["states"], "-p", out["pops"], "-d", out["fe"], "-b", out["nn"], "--batch", "300", *extra],
                       capture_output=True, text=True, timeout=300)
    return r, out


@pytest.mark.parametrize("D, path", [(10, "1..64 columns"), (100, "65..256 columns")])
def test_cli_assign_writes_what_the_python_path_gives(tmp_path, D, path):
    from clustering_amd import density
    R = cases.reference(D)
    Q = np.concatenate([cases.batch(R, N_NEW - 100, seed=3), cases.far_batch(R, 100, seed=4)])
    states = cases.states_of(len(R))
    radius = float(np.float32(cases.radius(D)))
    np.savetxt(tmp_path / "states", states, fmt="%d")
    np.save(tmp_path / "ref.npy", R)
    np.save(tmp_path / "new.npy", Q)
    write_ascii(tmp_path / "ref.txt", R)
    write_ascii(tmp_path / "new.txt", Q)

    r, out = assign(tmp_path, tmp_path / "ref.npy", tmp_path / "new.npy", tmp_path / "states", radius, "npy", "-v")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    frames = density.assign_frames_wide_pruned if D > 64 else density.assign_frames
    want = frames(torch.from_numpy(Q).cuda(), torch.from_numpy(R).cuda(), radius, states)
    w = {k: v.cpu().numpy() for k, v in want.items() if k != "max_pop"}
    assert f"served by: the resident reference of {path}" in r.stdout
    assert f"max_pop of the reference: {want['max_pop']}" in r.stdout
    assert data_lines(out["states"]) == ["%d" % s for s in w["states"]]
    assert data_lines(out["pops"]) == ["%d" % p for p in w["pops"]]
    assert data_lines(out["fe"]) == ["%e" % float(v) for v in w["fe"]]
    assert data_lines(out["nn"]) == ["%d %g %d %g" % (w["nn_idx"][i], float(w["nn_d2"][i]), w["hd_idx"][i], float(w["hd_d2"][i]))
                                     for i in range(N_NEW)]
    assert "inf" in data_lines(out["fe"]) and "0" in data_lines(out["states"]), "empty queries and the unassigned state occur"
    assert "#@   clustering_radius = %.5f" % np.float32(radius) in open(out["states"]).read()

    # ASCII inputs: identical files, the header's command line aside
    r, txt = assign(tmp_path, tmp_path / "ref.txt", tmp_path / "new.txt", tmp_path / "states", radius, "txt")
    assert r.returncode == 0, r.stderr[-2000:]
    for k in out:
        assert data_lines(txt[k]) == data_lines(out[k]), k


def test_cli_assign_refusals(tmp_path):
    R = cases.reference(10)
    np.save(tmp_path / "ref.npy", R)
    np.save(tmp_path / "new.npy", cases.batch(R, 50))
    np.save(tmp_path / "new3.npy", cases.batch(cases.reference(3), 50))
    np.savetxt(tmp_path / "states", cases.states_of(len(R)), fmt="%d")
    np.savetxt(tmp_path / "short", cases.states_of(len(R) - 1), fmt="%d")
    r, out = assign(tmp_path, tmp_path / "ref.npy", tmp_path / "new.npy", tmp_path / "short", cases.radius(10), "a")
    assert r.returncode != 0 and "state file does not match the number of reference frames" in r.stderr
    r, out = assign(tmp_path, tmp_path / "ref.npy", tmp_path / "new3.npy", tmp_path / "states", cases.radius(10), "b")
    assert r.returncode != 0 and "differ in their number of columns" in r.stderr
    assert not os.path.exists(out["states"])
    r, out = assign(tmp_path, tmp_path / "ref.npy", tmp_path / "none.npy", tmp_path / "states", cases.radius(10), "c")
    assert r.returncode != 0 and "cannot open file" in r.stderr
