"""The placement of the per-wave pruned sweeps' units (clustering_amd/csrc/dc_sweep_units.hpp): the decode (queue, ticket)
-> (block unit, share) is a bijection, the queue lengths add up, and every queue is the sequence its XCD label runs in
the static form (clustering_amd/bin/test_sweep_units, a host program)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_queues_are_the_static_sequences_and_cover_every_unit_once():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_sweep_units")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_sweep_units"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    # 9 block counts x 6 share counts: sum(n_blocks) * sum(n_chunks) units
    assert int(out.stdout.split()[1]) == (1 + 7 + 8 + 9 + 63 + 64 + 65 + 659 + 5209) * (1 + 2 + 7 + 8 + 10 + 64)
