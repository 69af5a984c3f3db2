"""GPU (-m gpu): the free-energy classes of the pruned neighbour sweep's reference tiles.

The early-out form of nn_pruned_kernel (rows of 5 - 10 columns) sorts the survivor tiles of a scan round by class --
nothing lower than any query of the wave, everything lower than every query, everything else -- and runs one loop per
class; the first two test against one cached threshold without looking at the tile's free-energy range.  Which class a
tile lands in depends on the free energies alone, so the cases below are free-energy patterns: all equal (every tile in
the first class, no lower neighbour anywhere), strictly increasing / decreasing with the row index, three distinct
values (the tile's minimum EQUAL to a query's free energy on many tiles: the strict < of the class rule), the real
pipeline's, and single query groups whose free-energy range lies below, above or around every other tile's.  Each
compares nn_idx, nn_d2 bits, hd_idx and hd_d2 bits of the default and the pruned variant with the direct kernels and
with the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


def two_blobs(n, D, seed):
    """two Gaussian blobs (sigma 0.08) a unit apart in the first column, a sixteenth of the rows duplicated (ties on
    d2: the lowest index wins)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.08, (n, D))
    x[:, 0] += rng.integers(0, 2, n)
    if n >= 64:
        x[rng.integers(0, n, n // 16)] = x[rng.integers(0, n, n // 16)]
    return np.ascontiguousarray(x, dtype=np.float32)


def pattern_fe(name, c, dens, seed=0):
    import torch
    n = c.shape[0]
    if name == "equal":
        return np.full(n, 1.25, np.float32)
    if name == "increasing":
        return (np.arange(n, dtype=np.float32) * np.float32(0.001)).astype(np.float32)
    if name == "decreasing":
        return ((n - np.arange(n, dtype=np.float32)) * np.float32(0.001)).astype(np.float32)
    if name == "three_values":
        return np.random.default_rng(seed).choice(np.array([0.5, 1.0, 2.0], np.float32), n).astype(np.float32)
    assert name == "pipeline"
    pops = dens.calculate_populations_partial(torch.from_numpy(c).cuda(), [0.2])
    return dens.calculate_free_energies(pops[0].contiguous()).cpu().numpy()


PATTERNS = ["equal", "increasing", "decreasing", "three_values", "pipeline"]


def same(got, exp, what):
    g = [t.cpu().numpy() for t in got]
    assert (g[0].astype(np.uint32).astype(np.uint64) == exp[0]).all(), (what, "nn_idx")
    assert (g[2].astype(np.uint32).astype(np.uint64) == exp[2]).all(), (what, "hd_idx")
    assert (bits(g[1]) == bits(exp[1])).all(), (what, "nn_d2")
    assert (bits(g[3]) == bits(exp[3])).all(), (what, "hd_d2")


def check(dens, oracle, c, fe, ranges, what):
    """all rows and the row ranges: default and pruned variant against the direct kernels and the oracle"""
    import torch
    ct, fet = torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda()
    for lo, hi in [(0, c.shape[0])] + list(ranges):
        exp = oracle.nearest_neighbors(c, fe, lo, hi)
        direct = dens.nearest_neighbors_partial(ct, fet, lo, hi, variant="direct")
        same(direct, exp, (what, lo, hi, "direct"))
        for variant in ("auto", "pruned"):
            got = dens.nearest_neighbors_partial(ct, fet, lo, hi, variant=variant)
            same(got, exp, (what, lo, hi, variant))
            for x, y, name in zip(got, direct, ("nn_idx", "nn_d2", "hd_idx", "hd_d2")):
                assert bool((x.view(torch.int32) == y.view(torch.int32)).all()), (what, lo, hi, variant, name)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_rows,D", [(4000, 10), (2500, 9), (3000, 4)], ids=["4000x10", "2500x9", "3000x4"])
def test_free_energy_patterns(dens, oracle, pattern, n_rows, D):
    """9 and 10 columns run the early-out form (two MFMAs per chain: the classes), 4 columns the full-chain form that
    has none; the row ranges cut cells and query groups"""
    c = two_blobs(n_rows, D, seed=n_rows + D)
    fe = pattern_fe(pattern, c, dens, seed=D)
    check(dens, oracle, c, fe, [(n_rows // 3, n_rows // 3 + n_rows // 2), (101, 101 + 50)], pattern)
    if pattern == "equal":
        hd = dens.nearest_neighbors_partial(*_dev(c, fe), variant="pruned")[2].cpu().numpy()
        assert (hd == n_rows + 1).all(), "no frame has a lower neighbour"


def _dev(c, fe):
    import torch
    return torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda()


@pytest.mark.parametrize("n_rows", [193, 6145])
@pytest.mark.parametrize("pattern", ["three_values", "pipeline", "increasing"])
def test_partly_padded_last_group_and_tile(dens, oracle, n_rows, pattern):
    """193 = six tiles and one row, 6145 = 192 tiles and one row: the last query group and the last reference tile are
    mostly pad rows (the last tile is kept out of the first two classes)"""
    c = two_blobs(n_rows, 10, seed=n_rows)
    fe = pattern_fe(pattern, c, dens, seed=n_rows)
    check(dens, oracle, c, fe, [(n_rows - 40, n_rows), (n_rows // 2, n_rows // 2 + 1)], (pattern, n_rows))


@pytest.mark.parametrize("where", ["around", "below", "above"])
def test_single_query_group_against_every_tile(dens, oracle, where):
    """one query group (a row range of 150 rows) whose free energies lie around, below or above those of every other
    row: every other tile then decides per lane, has nothing lower for the whole group, or is lower as a whole for
    the whole group"""
    n, lo, hi = 5000, 2100, 2250
    c = two_blobs(n, 10, seed=77)
    rng = np.random.default_rng(5)
    fe = rng.uniform(1.0, 2.0, n).astype(np.float32)
    if where == "around":
        fe[lo:hi] = np.where(np.arange(hi - lo) % 2 == 0, np.float32(0.5), np.float32(2.5))
    elif where == "below":
        fe[lo:hi] = rng.uniform(0.25, 0.5, hi - lo).astype(np.float32)
    else:
        fe[lo:hi] = rng.uniform(2.5, 3.0, hi - lo).astype(np.float32)
    check(dens, oracle, c, fe, [(lo, hi)], where)
    hd = oracle.nearest_neighbors(c, fe, lo, hi)[2][lo:hi]
    if where == "below":
        # (only the group's own rows can be lower)
        assert np.isin(hd[hd != n + 1], np.arange(lo, hi)).all()
    if where == "above":
        assert (hd != n + 1).all()


_COOP_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_nn_tile_classes as T
from clustering_amd import density as dens
from oracle.oracle import Oracle
oracle = Oracle()
for n, d in json.loads(sys.argv[2]):
    c = T.two_blobs(n, d, seed=n + d)
    for pattern in T.PATTERNS:
        fe = T.pattern_fe(pattern, c, dens, seed=d)
        ct, fet = torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda()
        exp = oracle.nearest_neighbors(c, fe)
        T.same(dens.nearest_neighbors_partial(ct, fet, variant="pruned"), exp, (n, d, pattern, "all rows"))
        lo, hi = n // 4, n // 4 + n // 3
        T.same(dens.nearest_neighbors_partial(ct, fet, lo, hi, variant="pruned"), oracle.nearest_neighbors(c, fe, lo, hi),
               (n, d, pattern, "row range"))
        words = None
        for g in range(3):
            w = dens.pack_neighbors(*dens.nearest_neighbors_segment(ct, fet, g, 3))
            words = w if words is None else torch.minimum(words, w)
        T.same(dens.unpack_neighbors(words), exp, (n, d, pattern, "segments"))
print("ok")
"""


@pytest.mark.parametrize("extra", [{"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "8"}, {"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "16"}],
                         ids=["floor 8", "floor 16"])
def test_cooperative_shares(extra):
    """the instance whose waves are the shares of one query group, forced on in a process of its own (the switches are
    read once per process): every pattern, all rows, a row range and three segments against the oracle"""
    r = subprocess.run([sys.executable, "-c", _COOP_CHILD, ROOT, json.dumps([(3000, 10), (2049, 9)])],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, **extra))
    assert r.returncode == 0 and "ok" in r.stdout, (extra, r.stdout[-1000:], r.stderr[-3000:])
