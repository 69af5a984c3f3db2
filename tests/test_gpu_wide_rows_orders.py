"""The avx and fma builds of the library (clustering_amd/lib_avx, lib_fma: DC_CANON_ORDER=avx / fma) on rows wider than
400 columns (dc_wide.hip keeps 8 lane sums per pair there) against the oracle of the same order, bit for bit -- in a
child process, since a process binds one build of the library."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from clustering_amd import capi, density as dens
from clustering_amd.synth import gaussian_blobs
from oracle.oracle import Oracle
ORDER = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == ORDER
o, o_def = Oracle(order=ORDER), Oracle()
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
u64 = lambda t: t.cpu().numpy().astype(np.uint32).astype(np.uint64)
differ = 0   # rows whose neighbour d2 under this order differs from the default order's, in bits
for n, d in [(700, 401), (500, 407), (600, 408), (400, 1000), (300, 1031)]:
    c = gaussian_blobs(n, d, seed=950 + d)
    c[: n // 9] = c[n // 3: n // 3 + n // 9]          # duplicates: ties at distance 0
    ct = torch.from_numpy(c).cuda()
    r = float(np.float32(0.08 * np.sqrt(2.0 * d)))
    radii = [r, r * 1.2, r * 0.8]
    want = o.populations(c, radii)
    fe_want = o.free_energies(want[0])
    exp = o.nearest_neighbors(c, fe_want)
    differ += int((bits(exp[1]) != bits(o_def.nearest_neighbors(c, fe_want)[1])).sum())
    for v in ("direct", "auto"):
        p = dens.calculate_populations_partial(ct, radii, variant=v)
        assert (u64(p) == want).all(), (n, d, v, "pops")
        fe = dens.calculate_free_energies(p[0].contiguous())
        assert (bits(fe.cpu().numpy()) == bits(fe_want)).all(), (n, d, v, "fe")
        g = [t.cpu().numpy() for t in dens.nearest_neighbors_partial(ct, fe, variant=v)]
        assert (g[0].astype(np.uint32).astype(np.uint64) == exp[0]).all(), (n, d, v, "nn idx")
        assert (g[2].astype(np.uint32).astype(np.uint64) == exp[2]).all(), (n, d, v, "nn_hd idx")
        assert (bits(g[1]) == bits(exp[1])).all() and (bits(g[3]) == bits(exp[3])).all(), (n, d, v, "nn d2")
    acc = torch.zeros_like(p)
    for s in range(3):
        acc += dens.calculate_populations_segment(ct, radii, s, 3)
    assert (u64(acc) == want).all(), (n, d, "segments")
    # the radius graph: every pair once, and the degrees of the list are the oracle's populations
    r2 = np.float32(np.float32(r) * np.float32(r))
    pairs, pops = dens.radius_pairs(ct, r2)
    pl = pairs.cpu().numpy().astype(np.int64)
    assert (pl[:, 0] < pl[:, 1]).all() and len(np.unique(pl[:, 0] * n + pl[:, 1])) == len(pl), (n, d, "pairs")
    deg = np.ones(n, dtype=np.uint64)
    np.add.at(deg, pl[:, 0], 1)
    np.add.at(deg, pl[:, 1], 1)
    assert (deg == want[0]).all() and (pops.cpu().numpy().astype(np.uint64) == want[0]).all(), (n, d, "pair pops")
assert differ > 0, "the order-specific oracle gave the default order's neighbour distances everywhere"
print("ok: neighbour d2 under the two orders differ in", differ, "rows")
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_other_order_library_on_wide_rows(order):
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ok:" in r.stdout
