"""GPU (-m gpu): the reference-side credit of the symmetric one-radius population sweep (dc_credit.hpp) on
inputs chosen to load it, against the CPU oracle, bit for bit.  The sweep credits BOTH frames of a pair that a wave meets
outside its own query group: the query side in-lane, the reference side through the lane network -- whose arithmetic
tests/test_credit_model.py checks on emulated lanes; what is left for the device is whether the hardware's exchanges
and the kernels around them give the same counts.

  duplicates   several thousand copies of one row among blobs: whole tile pairs inside, every (lane, element) count of a
               reference tile at 6 and the row sums at 192 = 6 query tiles x 32 lanes -- the largest a byte has to carry
  ball         all rows inside one another's radius: nothing is pruned, every count is n, and the number of evaluated
               tiles (10 columns) shows that every unordered pair of groups was met ONCE: the symmetric sweep, not the one-sided one
  lattice      integer coordinates, r^2 an integer d2 level: pairs AT the radius stay outside (the strict <)
  shapes       n_rows off the multiples of 32 and of 192 (pad rows, pad tiles of the last query group); 3, 10, 16 and 26
               columns (1, 2, 4, 5 MFMAs per chain)
  segments     the partial counts of 2 and of 8 segments add up to the oracle's
  forms        variants `pruned` and `auto` here; the shared-operand sweep (pop_shared_kernel, the same credit per radius)
               forced on in a child process at 26 and 30 columns, where it is built
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (3, 10, 16, 26)


def duplicates(n, d, seed, copies):
    """blobs with `copies` rows replaced by one and the same row, scattered over the caller's order"""
    from clustering_amd.synth import gaussian_blobs
    c = gaussian_blobs(n, d, seed=seed)
    rng = np.random.default_rng(seed)
    where = rng.permutation(n)[:copies]
    c[where] = c[where[0]]
    return c


def ball(n, d, seed, r):
    """n rows within r / 4 of the origin in every direction: every pair is well inside r"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, d)) * (r / (4.0 * np.sqrt(d)))
    c[: n // 2] = c[0]     # half of them one row
    return c.astype(np.float32)


def lattice(n, d, seed):
    """integer coordinates in -1 .. 4 (every d2 an integer, exact in any summation order)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, (max(1, n // 4), d))
    rows = base[rng.integers(0, len(base), n)]
    step = rng.choice([-1, 0, 1], size=(n, d), p=[0.5 / (d + 1), 1.0 - 1.0 / (d + 1), 0.5 / (d + 1)])
    return (rows + step).astype(np.float32)


def cases():
    """(name, coords, radius): sizes off the multiples of 32 and 192 except where noted"""
    out = []
    for k, d in enumerate(WIDTHS):
        n = (6000 + 17, 5000 + 1, 4097, 6144 + 33)[k]          # 6144 = 32 * 192: one row into the next tile and group
        out.append((f"duplicates-D{d}-n{n}", duplicates(n, d, 11 + d, 3000 + 100 * k), 0.2 + 0.02 * d))
        out.append((f"lattice-D{d}-n{n - 900}", lattice(n - 900, d, 5 + d), (1.0, 2.0, 2.0, 2.0)[k]))
    out.append(("ball-D10-n6144", ball(6144, 10, 3, 0.5), 0.5))   # whole tiles and groups, no pad anywhere
    out.append(("ball-D26-n3001", ball(3001, 26, 4, 0.5), 0.5))
    return out


CASES = cases()


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


@pytest.fixture(scope="module")
def want():
    """the oracle's populations of every case, computed once"""
    from oracle.oracle import Oracle
    o = Oracle()
    return {name: o.populations(c, [r])[0] for name, c, r in CASES}


def as_u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


def test_the_cases_load_the_credit(want):
    """conditions of the cases, from the oracle's side: the duplicated rows see thousands of frames, the lattices have
    pairs exactly at the radius, the balls are complete"""
    for name, c, r in CASES:
        if name.startswith("duplicates"):
            assert int(want[name].max()) >= 3000, name           # >= 93 tiles of copies: reference tiles wholly inside
        if name.startswith("ball"):
            assert (want[name] == len(c)).all(), name
        if name.startswith("lattice"):
            d2 = ((c[:200, None, :].astype(np.float64) - c[None, :, :]) ** 2).sum(axis=2)   # (integers: exact)
            assert (d2 == r * r).any() and (d2 < r * r).any() and (d2 > r * r).any(), name
        assert len(c) % 32 != 0 or name == "ball-D10-n6144", name


@pytest.mark.parametrize("variant", ["pruned", "auto"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_all_rows_against_the_oracle(dens, want, case, variant):
    import torch
    name, c, r = case
    ct = torch.from_numpy(c).cuda()
    got = as_u64(dens.calculate_populations_partial(ct, [r], variant=variant)[0])
    tiles = dens.evaluated_tiles(ct.device)[0]
    bad = np.nonzero(got != want[name])[0]
    print(f"credit: {name} {variant}: max count {int(want[name].max())}, tiles {tiles}, rows off {len(bad)}", flush=True)
    assert len(bad) == 0, (name, variant, bad[:8], got[bad[:8]], want[name][bad[:8]])
    assert tiles > 0, (name, variant, "the matrix-core sweep did not run")
    if name == "ball-D10-n6144":
        # nothing can be pruned.  T = 192 tiles in 32 groups of 6: the symmetric sweep meets the 6 x 6 tile pairs of a
        # group with itself and every other group once, T^2 / 2 + 6 T tile pairs (as much again allowed for as slack);
        # a one-sided sweep meets T^2
        T = len(c) // 32
        assert tiles <= T * T // 2 + 12 * T < T * T, (name, variant, tiles, T)


@pytest.mark.parametrize("n_seg", [2, 8])
@pytest.mark.parametrize("name", ["duplicates-D10-n5001", "lattice-D26-n5277"])
def test_segments_add_up(dens, want, name, n_seg):
    import torch
    c, r = next((c, r) for nm, c, r in CASES if nm == name)
    ct = torch.from_numpy(c).cuda()
    acc = np.zeros(len(c), dtype=np.uint64)
    for g in range(n_seg):
        acc += as_u64(dens.calculate_populations_segment(ct, [r], g, n_seg)[0])
    bad = np.nonzero(acc != want[name])[0]
    print(f"credit: {name}: {n_seg} segments, rows off {len(bad)}", flush=True)
    assert len(bad) == 0, (name, n_seg, bad[:8], acc[bad[:8]], want[name][bad[:8]])


SHARED_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
from clustering_amd import density as dens
from oracle.oracle import Oracle
import test_gpu_credit as G
o = Oracle()
for name, c, r in [("duplicates-D26", G.duplicates(6144 + 33, 26, 37, 3300), 0.72), ("lattice-D26", G.lattice(5277, 26, 31), 2.0),
                   ("ball-D26", G.ball(3001, 26, 4, 0.5), 0.5), ("duplicates-D30", G.duplicates(4097, 30, 41, 3000), 0.8)]:
    want = o.populations(c, [r])[0]
    ct = torch.from_numpy(c).cuda()
    for variant in ("pruned", "auto"):
        got = G.as_u64(dens.calculate_populations_partial(ct, [r], variant=variant)[0])
        assert dens.evaluated_tiles(ct.device)[0] > 0, (name, variant)
        assert (got == want).all(), (name, variant, np.nonzero(got != want)[0][:8])
    for n_seg in (2, 8):
        acc = np.zeros(len(c), dtype=np.uint64)
        for g in range(n_seg):
            acc += G.as_u64(dens.calculate_populations_segment(ct, [r], g, n_seg)[0])
        assert (acc == want).all(), (name, n_seg, np.nonzero(acc != want)[0][:8])
    print("credit (shared operands):", name, "max count", int(want.max()), file=sys.stderr)
print("ok")
"""


def test_shared_operand_form():
    """pop_shared_kernel<..., SYM> forced on (DC_POP_SHARED=1 is read once per process: a child) where it is built for one
    radius, 5 and 6 MFMAs per chain"""
    r = subprocess.run([sys.executable, "-c", SHARED_CHILD, ROOT], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, DC_POP_SHARED="1"))
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]
