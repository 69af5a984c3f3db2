"""GPU: the chain of the matrix-core sweeps at 257..1024 columns end to end (tests/cpp/test_xwide_model.hip, built with the
library): every accumulator within e0 + kappa S d2 of S d2 at D = 257, 512, 1024 and data scales 1e-3 .. 1e3; every one of
1024 column means in the workspace (a column the statistics pass leaves at 0 costs no wrong result anywhere, only band
pairs: this is the one place that reads the means back); and the last-chunk rule at NM = 49, 50, 51, 52 against a chain
that runs one MFMA at a time."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_xwide_chain_band_means_and_last_chunk():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_xwide_model")
    assert os.path.exists(exe), "__graft_entry__.build() makes it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout[-3000:] + r.stderr[-2000:]
    ratios = [float(x) for x in re.findall(r"worst \|err\|/band = ([0-9.eE+-]+)", r.stdout)]
    assert len(ratios) == 9 and max(ratios) <= 1.0
    assert re.search(r"means D=1024: 0 of 1024 columns off", r.stdout)
    chunks = re.findall(r"chunks D=(\d+) NM=(\d+) \(NM mod 4 = (\d)\): (\d+) of", r.stdout)
    assert [(int(d), int(nm), int(rem), int(bad)) for d, nm, rem, bad in chunks] == \
        [(257, 49, 1, 0), (261, 50, 2, 0), (267, 51, 3, 0), (272, 52, 0, 0)]
