"""GPU: the chain of the wide matrix-core sweeps end to end against its band (tests/cpp/test_wide_model.hip, built with the
library): D = 65, 128, 256 on clustered data at scales 1e-3 .. 1e3, every accumulator within e0 + kappa S d2 of S d2."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_chain_stays_within_its_band():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_model")
    assert os.path.exists(exe), "__graft_entry__.build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-3000:] + r.stderr[-2000:]
    ratios = [float(x) for x in re.findall(r"worst \|err\|/band = ([0-9.eE+-]+)", r.stdout)]
    assert len(ratios) == 9 and max(ratios) <= 1.0
