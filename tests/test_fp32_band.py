"""CPU: runs the host program tests/cpp/test_fp32_band.cpp (built by the library's Makefile into clustering_amd/bin): the
guard band and the image scale of the fp32-input MFMA sweeps for chains of 1..16 K-steps and both parities of the column
count, against long double arithmetic."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_and_scale_hold_for_every_chain_length():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_fp32_band")
    assert os.path.exists(exe), "build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout[-3000:] + r.stderr[-1000:]
    assert "S = 1..16" in r.stdout
