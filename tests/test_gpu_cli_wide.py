"""GPU: `clustering density` on 100 columns with and without DC_SESSION_WIDE=1, and with the variable on two "devices" of
the one GPU (DC_SESSION_DEVICES=0,0): every output file -- populations and free energies per radius (-R), and populations,
free energies, neighbours and the screening's clusterings of one radius (-r -b -T -o) -- is byte-identical between the
three runs (but for the line of the header that holds the time of the run), the populations are the CPU oracle's, and under -v the line that names the sweeps of the session differs."""
import os
import subprocess

import numpy as np
import pytest

import widepruneref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "clustering_amd", "bin", "clustering")
RUNS = {"default": {}, "wide": {"DC_SESSION_WIDE": "1"},
        "wide, two devices": {"DC_SESSION_WIDE": "1", "DC_SESSION_DEVICES": "0,0", "DC_SESSION_ALLOW_DUPLICATE_DEVICES": "1"}}


def content(path):
    """every byte of a file but the one line of its header that holds the time of the run ("# Created ...")"""
    lines = open(path, "rb").read().split(b"\n")
    stamps = [l for l in lines if l.startswith(b"# Created ")]
    assert len(stamps) == 1, (path, stamps)
    return b"\n".join(l for l in lines if not l.startswith(b"# Created "))


def run(out_dir, coords, radii, extra_env):
    """both invocations of one run into out_dir -> (file name -> bytes, the -v lines that name the sweeps)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DC_SESSION_")}
    env.update(extra_env)
    os.makedirs(out_dir)
    p = lambda name: name      # (relative to the run's own directory: the command lines of the runs are the same text)
    several = [CLI, "density", "-f", coords, "-R", *[repr(float(r)) for r in radii], "-p", p("pops"), "-d", p("fes"), "-v"]
    one = [CLI, "density", "-f", coords, "-r", repr(float(radii[0])), "-p", p("pop"), "-d", p("fe"), "-b", p("nn"),
           "-T", "0.5", "0.75", "3.0", "-o", p("clust"), "-v"]
    lines = []
    for cmd in (several, one):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=out_dir)
        assert r.returncode == 0, r.stderr + r.stdout[-2000:]
        lines += [l for l in r.stdout.splitlines() if l.startswith("sweeps: ")]
    return {name: content(os.path.join(out_dir, name)) for name in sorted(os.listdir(out_dir))}, lines


def test_output_files_are_identical_and_the_verbose_line_differs(tmp_path, oracle):
    c = pr.stretched(1500, 100)
    np.save(tmp_path / "c.npy", c)
    radii = pr.radii_for(100, 3)
    got = {name: run(str(tmp_path / name.replace(", ", "_").replace(" ", "_")), str(tmp_path / "c.npy"), radii, env)
           for name, env in RUNS.items()}
    files, lines = got["default"]
    assert len(files) >= 3 + 3 + 3 + 2, sorted(files)      # pops and fes of 3 radii, pop / fe / nn, the clusterings
    assert any(name.startswith("clust.") for name in files) and "nn" in files
    for name in ("wide", "wide, two devices"):
        other, other_lines = got[name]
        assert sorted(other) == sorted(files), name
        for f in files:
            assert other[f] == files[f], (name, f, "differs from the default session's file")
        assert len(other_lines) == 2 and all("pruned wide matrix-core sweeps" in l for l in other_lines), other_lines
    assert len(lines) == 2 and all("default sweeps" in l for l in lines) and lines[0] != got["wide"][1][0]
    # ... and the files hold the oracle's numbers
    pops = oracle.populations(c, radii)
    text = [l for l in files["pop"].decode().splitlines() if l and not l.startswith("#")]
    assert text == [str(int(v)) for v in pops[0]]
    for k, r in enumerate(radii):
        text = [l for l in files["pops_%f" % np.float32(r)].decode().splitlines() if l and not l.startswith("#")]
        assert text == [str(int(v)) for v in pops[k]], r
