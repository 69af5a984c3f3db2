"""The radial gap of the pruned neighbour sweep's ring rule (clustering_amd/csrc/dc_rho_gap.hpp).

With rho(x) = |(x - o)[2..D)|, o the origin of the frame's component, two frames of one component are at least
sqrt(d2_01 + (rho(x) - rho(y))^2) apart; every reference tile keeps the range of rho over its rows, and the ring scan
of nn_pruned_kernel adds the squared gap between the tile's range and the query group's to the box gap in columns 0/1.
The term only ever removes tile pairs: DC_NN_RHO=0 passes no ranges and must give the same four arrays.

GPU (-m gpu).  Every case runs all rows, the segments of world size 2 and 3 (merged like a sharded run merges them) and
a row range (its own query order: no ranges, the counter as without the term), with variant "pruned", and holds nn_idx,
nn_d2 bits, hd_idx and hd_d2 bits to the CPU oracle.  The same calls run under DC_NN_RHO=0 in a fresh child process
(the switches are read once per process); the arrays must be equal and the kernel's tile-pair counter
(density.evaluated_tiles) with the term must not exceed the counter without it -- on the shells it must be strictly lower.
The cooperative form of the kernel (DC_NN_COOP=1, small shares) runs in children of its own, with and without the term.
There the shares of a query group run at the same time and learn incumbents from each other while they sweep, so the
counter of one and the same library moves by a per cent or two from run to run (the three components, where the
deterministic form shows that the term removes nothing: 16 380 against 16 704 tile pairs for all rows, 18 006 against
17 856 for two segments, two runs a moment apart).  A comparison of two such runs says something only where the term
removes more than that spread: the counters of the cooperative form are compared on the shells (a quarter fewer tile
pairs) and printed for the components; the arrays are held to the oracle and to each other in both.

CPU: tests/cpp/test_rho_gap.cpp holds the header's rounding rule to double arithmetic on 10^6 interval pairs."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KINDS = ("all", "seg2", "seg3", "range")
NAMES = ("nn_idx", "nn_d2", "hd_idx", "hd_d2")


# ---- the cases: name -> (coords, free energies, row range) -----------------------------------------------------------
def _directions(rng, n, d):
    v = rng.normal(0.0, 1.0, (n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def shells(D, seed):
    """6 000 rows.  Columns 0/1 are one point of the plane for all but four far rows (which give the plane an extent, so
    that the cell edge -- the first ring -- is about 0.02: everything else sits in ONE cell); the other columns lie on two
    thin shells rho = 0.1 and rho = 0.3 around the centre.  Eight frames lie between the shells at rho = 0.2 on the ray of
    one frame of either shell: their nearest neighbours are those two, at a distance EQUAL to the radial difference
    (collinear rest-vectors: the boundary of the bound); half of them come three times (a tie at d2 = 0: the lowest index)."""
    rng = np.random.default_rng(seed)
    n, n_far, n_mid = 6000, 4, 8
    n_dup = 2 * (n_mid // 2)
    n_shell = n - n_far - n_mid - n_dup
    u = _directions(rng, n_shell, D - 2)
    rho = np.where(np.arange(n_shell) % 2 == 0, 0.1, 0.3)
    rest = u * rho[:, None]
    # the rays of the frames in between: each has a frame on both shells
    for i in range(n_mid):
        rest[2 * i] = 0.1 * u[2 * i]
        rest[2 * i + 1] = 0.3 * u[2 * i]
    mid = np.stack([0.2 * u[2 * i] for i in range(n_mid)])
    dup = np.concatenate([mid[: n_mid // 2], mid[: n_mid // 2]])
    far = rng.normal(0.0, 0.05, (n_far, D - 2))
    body = np.concatenate([rest, mid, dup, far])
    c = np.zeros((n, D))
    c[:, 0] = 0.5
    c[:, 1] = -0.25
    c[:, 2:] = body + 0.7          # (a centre away from zero)
    c[n - n_far:, 0] = 1.5
    perm = rng.permutation(n)
    c = np.ascontiguousarray(c[perm], dtype=np.float32)
    fe = (4.0 * np.linalg.norm(body, axis=1))[perm].astype(np.float32)
    return c, fe, (1000, 1700)


def blobs(n, D, seed):
    """two Gaussian blobs (sigma 0.08) a unit apart in the first column, a sixteenth of the rows duplicated"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.08, (n, D))
    x[:, 0] += rng.integers(0, 2, n)
    x[rng.integers(0, n, n // 16)] = x[rng.integers(0, n, n // 16)]
    return np.ascontiguousarray(x, dtype=np.float32)


def radial_fe(c, sign):
    """a free energy that grows (sign > 0) or falls with the distance from the blob's centre in the columns behind 0/1"""
    ctr = np.round(c[:, :1].astype(np.float64))
    rest = c[:, 2:].astype(np.float64)
    rho = np.linalg.norm(rest, axis=1) if c.shape[1] > 2 else np.abs(c[:, 0] - ctr[:, 0])
    return (2.0 + sign * 3.0 * rho).astype(np.float32)


def three_components(seed):
    """4 999 rows (the last tile has pad rows) in three blobs three units apart: components with origins of their own,
    one of 150 rows -- less than a query group of 192"""
    rng = np.random.default_rng(seed)
    sizes, D = (150, 2400, 2449), 10
    parts, rhos = [], []
    for k, m in enumerate(sizes):
        x = rng.normal(0.0, 0.06, (m, D))
        rhos.append(np.linalg.norm(x[:, 2:], axis=1))
        x[:, 0] += 3.0 * k
        x[:, 1] -= 1.0 * k
        x[:, 2:] += 0.25 * (k + 1)
        parts.append(x)
    c, rho = np.concatenate(parts), np.concatenate(rhos)
    perm = rng.permutation(c.shape[0])
    return np.ascontiguousarray(c[perm], dtype=np.float32), (1.0 + 5.0 * rho[perm]).astype(np.float32), (2000, 2300)


def make_case(name):
    if name == "shells3":
        return shells(3, seed=3)
    if name == "shells10":
        return shells(10, seed=10)
    if name == "cols2":
        c = blobs(3000, 2, seed=2)
        return c, radial_fe(c, +1.0), (700, 1500)
    if name == "cols3":
        c = blobs(3000, 3, seed=33)
        return c, radial_fe(c, +1.0), (700, 1500)
    if name == "anticorrelated":
        c = blobs(4000, 10, seed=4)
        return c, radial_fe(c, -1.0), (900, 2100)
    if name == "random_fe":
        c = blobs(4000, 10, seed=5)
        return c, np.random.default_rng(6).uniform(1.0, 3.0, 4000).astype(np.float32), (900, 2100)
    assert name == "components"
    return three_components(seed=7)


CASES = ("shells3", "shells10", "cols2", "cols3", "anticorrelated", "random_fe", "components")
COOP_CASES = ("shells10", "components")
COOP_ENV = {"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "8"}


# ---- one case on the device: the four kinds of call, their arrays and tile-pair counters -----------------------------
def run_case(dens, name):
    import torch
    c, fe, (lo, hi) = make_case(name)
    ct, fet = torch.from_numpy(c).cuda(), torch.from_numpy(fe).cuda()
    dev = ct.device
    out = {}

    def keep(kind, arrays, tiles):
        for nm, a in zip(NAMES, arrays):
            out[kind + "." + nm] = a.cpu().numpy().view(np.uint32)
        out[kind + ".tiles"] = np.array([tiles], np.int64)

    got = dens.nearest_neighbors_partial(ct, fet, variant="pruned")
    keep("all", got, dens.evaluated_tiles(dev)[1])
    for world in (2, 3):
        words, tiles = None, 0
        for g in range(world):
            w = dens.pack_neighbors(*dens.nearest_neighbors_segment(ct, fet, g, world, variant="pruned"))
            tiles += dens.evaluated_tiles(dev)[1]
            words = w if words is None else torch.minimum(words, w)
        keep("seg%d" % world, dens.unpack_neighbors(words), tiles)
    got = dens.nearest_neighbors_partial(ct, fet, lo, hi, variant="pruned")
    keep("range", got, dens.evaluated_tiles(dev)[1])
    return out


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_nn_radial_gap as T
from clustering_amd import density as dens
out = {}
for name in json.loads(sys.argv[2]):
    for k, v in T.run_case(dens, name).items():
        out[name + "/" + k] = v
np.savez(sys.argv[3], **out)
print("ok")
"""


def child(path, names, env):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(list(names)), path], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and "ok" in r.stdout, (env, r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in names}


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


@pytest.fixture(scope="module")
def without_term(tmp_path_factory):
    """every case under DC_NN_RHO=0, in ONE fresh child process"""
    return child(str(tmp_path_factory.mktemp("rho") / "off.npz"), CASES, {"DC_NN_RHO": "0"})


@pytest.fixture(scope="module")
def coop(tmp_path_factory):
    """the cooperative form, with and without the term: a child each"""
    d = tmp_path_factory.mktemp("rho_coop")
    return (child(str(d / "on.npz"), COOP_CASES, dict(COOP_ENV)),
            child(str(d / "off.npz"), COOP_CASES, dict(COOP_ENV, DC_NN_RHO="0")))


_expected = {}


def expected(oracle, name):
    """the oracle's answers of a case, computed once"""
    if name not in _expected:
        c, fe, (lo, hi) = make_case(name)
        _expected[name] = (oracle.nearest_neighbors(c, fe), oracle.nearest_neighbors(c, fe, lo, hi))
    return _expected[name]


def hold(oracle, name, on, off, strict, counters=True):
    full, part = expected(oracle, name)
    for kind in KINDS:
        exp = part if kind == "range" else full
        want = (exp[0].astype(np.uint32), np.ascontiguousarray(exp[1], np.float32).view(np.uint32),
                exp[2].astype(np.uint32), np.ascontiguousarray(exp[3], np.float32).view(np.uint32))
        for nm, w in zip(NAMES, want):
            assert (on[kind + "." + nm] == w).all(), (name, kind, nm, "against the oracle")
            assert (off[kind + "." + nm] == w).all(), (name, kind, nm, "DC_NN_RHO=0 against the oracle")
            assert (on[kind + "." + nm] == off[kind + "." + nm]).all(), (name, kind, nm, "with against without the term")
        t_on, t_off = int(on[kind + ".tiles"][0]), int(off[kind + ".tiles"][0])
        print("%s %s: tile pairs %d with the term, %d without" % (name, kind, t_on, t_off))
        assert t_off > 0 and t_on > 0, (name, kind)
        if not counters:
            continue
        assert t_on <= t_off, (name, kind, t_on, t_off)
        if strict and kind != "range":
            assert t_on < t_off, (name, kind, t_on, t_off)
    return on, off


@gpu
@pytest.mark.parametrize("D", [3, 10])
def test_shells(dens, oracle, without_term, D):
    """the group of a shell never looks at the other shell's tiles once its own neighbours are confirmed: strictly
    fewer tile pairs; the frames between the shells find their neighbours at exactly the radial difference"""
    name = "shells%d" % D
    on, _ = hold(oracle, name, run_case(dens, name), without_term[name], strict=True)
    c, fe, _ = make_case(name)
    rest = c[:, 2:].astype(np.float64) - 0.7
    rho = np.linalg.norm(rest, axis=1)
    mid = np.flatnonzero((np.abs(rho - 0.2) < 0.01) & (c[:, 0] < 1.0))
    assert len(mid) == 16
    nn = on["all.nn_idx"][mid].astype(np.int64)
    d2 = on["all.nn_d2"][mid].view(np.float32)
    dups = d2 == 0.0
    if D == 10:
        assert dups.sum() == 12   # (four frames in three copies; at three columns a ray is a sign: all are copies)
    assert (np.abs(np.sqrt(d2[~dups]) - 0.1) < 1e-5).all()
    # a neighbour in a shell lies on the frame's own ray; a copy's neighbour is the lowest other index among its copies
    for i, j, is_dup in zip(mid, nn, dups):
        if is_dup:
            same = np.flatnonzero((c == c[i]).all(axis=1))
            assert j == min(k for k in same if k != i)
        else:
            assert abs(abs(rho[j] - 0.2) - 0.1) < 1e-5 and np.allclose(rest[j] / rho[j], rest[i] / rho[i], atol=1e-4)


@gpu
@pytest.mark.parametrize("name", ["cols2", "cols3"])
def test_two_and_three_columns(dens, oracle, without_term, name):
    """two columns: no columns behind the cell grid, the ranges are (0, 0) and the counters equal; three: rho = |x2 - o2|"""
    on, off = hold(oracle, name, run_case(dens, name), without_term[name], strict=False)
    if name == "cols2":
        assert all(int(on[k + ".tiles"][0]) == int(off[k + ".tiles"][0]) for k in KINDS)


@gpu
@pytest.mark.parametrize("name", ["anticorrelated", "random_fe"])
def test_tiles_wide_in_rho(dens, oracle, without_term, name):
    """free energies falling with rho, or random: the order does not make tiles thin shells, little or nothing is pruned"""
    hold(oracle, name, run_case(dens, name), without_term[name], strict=False)


@gpu
def test_three_components(dens, oracle, without_term):
    """origins per component, a component inside one query group, pad rows in the last tile"""
    on, off = hold(oracle, "components", run_case(dens, "components"), without_term["components"], strict=False)
    # (a row range has an order of its own: no ranges, the same tile pairs)
    assert int(on["range.tiles"][0]) == int(off["range.tiles"][0])


@gpu
@pytest.mark.parametrize("name", COOP_CASES)
def test_cooperative_shares(oracle, coop, name):
    """DC_NN_COOP=1 with shares of eight tiles: the waves of a workgroup are shares of one query group"""
    hold(oracle, name, coop[0][name], coop[1][name], strict=(name == "shells10"), counters=(name == "shells10"))


# ---- CPU: the rounding rule ---------------------------------------------------------------------------------------------
def test_rounding_rule_on_the_host(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "the rounding rule is checked by a host program: g++ is needed"
    exe = str(tmp_path / "test_rho_gap")
    r = subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "clustering_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_rho_gap.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    words = r.stdout.split()
    assert r.returncode == 0 and words[-1] == "OK", r.stdout[-2000:] + r.stderr[-2000:]
    figures = {words[i]: int(words[i + 1]) for i in range(0, 10, 2)}
    assert figures["pairs"] == 1000000
    assert figures["contain_failures"] == 0 and figures["gap_failures"] == 0 and figures["empty_failures"] == 0
    # (not vacuous: a third of the pairs have a positive gap)
    assert figures["positive"] > 200000
