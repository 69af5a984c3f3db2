"""The workspace layout of the resident reference at 65..1024 columns (clustering_amd/csrc/dc_mfma_wide.hip
wide_reference_layout): every array inside the total and none over another, the resident region
behind the means of the width's layout, the three regions disjoint, the words per query block where the launcher puts them,
the unit map of the pruned cross sweep, and up to 256 columns the recorded byte offsets
(clustering_amd/bin/test_reference_xwide_layout, a host program: tests/cpp/test_reference_xwide_layout.hip)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_layout_of_the_grid_holds():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_reference_xwide_layout")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_reference_xwide_layout"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    # 9 widths x 6 reference counts x 6 batch sizes, three batches each, and the five recorded layouts
    assert int(out.stdout.split()[1]) == 9 * 6 * 6 * 3 + 5
