"""The workspace ranges of the radius graph and the neighbour blocks at 257..1024 columns (clustering_amd/csrc/dc_mfma_wide.hip,
DESIGN.md 4.37): every byte range the six graph launchers and the three block launchers address -- images, norms, the
order, boxes, rows 0..2 of the count region, the order's signature and hash words, the layout-status word -- lies inside
what dc_hip_xwide_workspace_bytes / dc_hip_xwide_pruned_workspace_bytes hand out, the words of the header do not run into
the images, and every (query block, share) unit of a segment's launch is met once (clustering_amd/bin/test_xwide_graph_layout,
a host program built from the library's own layout functions: tests/cpp/test_xwide_graph_layout.hip)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_layout_of_the_grid_holds():
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_xwide_graph_layout")
    assert os.path.exists(exe), "build() makes clustering_amd/bin/test_xwide_graph_layout"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    # rows 1 .. 70 000 x 8 column counts x 5 segment counts
    assert int(out.stdout.split()[1]) == 70000 * 8 * 5
