"""CPU: bench.py --dump-outputs (what the timed path computed, as .npy files within a fixed budget) and --steps."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def outputs(n, n_radii, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"pops": torch.randint(1, n + 1, (n_radii, n), dtype=torch.int32, generator=g),
            "fe": torch.rand(n, generator=g), "nn_idx": torch.randint(0, n + 2, (n,), dtype=torch.int32, generator=g),
            "nn_d2": torch.rand(n, generator=g), "hd_idx": torch.randint(0, n + 2, (n,), dtype=torch.int32, generator=g),
            "hd_d2": torch.full((n,), float(np.finfo(np.float32).max))}


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_is_exact_float32_or_float64(tmp_path):
    out = outputs(1000, 2)
    bench.dump_outputs(out, 1000, str(tmp_path / "d"))
    got = load(tmp_path / "d")
    assert sorted(got) == sorted(out)
    for k, a in got.items():
        assert a.dtype in (np.float32, np.float64), k
        assert a.shape == tuple(out[k].shape) and (a == out[k].numpy()).all(), k


def test_dump_over_budget_keeps_the_same_seeded_rows(tmp_path, monkeypatch):
    n = 5000
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 40_000)
    out = outputs(n, 3)
    for d in ("a", "b"):
        bench.dump_outputs(out, n, str(tmp_path / d))
    a, b = load(tmp_path / "a"), load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 40_000
    rows = a["rows"].astype(np.int64)
    assert 0 < rows.size < n and (np.diff(rows) > 0).all()
    for k in out:
        assert a[k].shape[-1] == rows.size and (a[k] == out[k].numpy()[..., rows]).all(), k
    for k in a:
        assert (a[k] == b[k]).all(), k


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
