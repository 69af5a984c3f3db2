"""GPU (-m gpu): the neighbour sweeps driven with free energies of any origin (tests/fe_families.py), against the CPU
oracle -- nn_idx and hd_idx equal, nn_d2 and hd_d2 bit for bit.

Every other neighbour test hands in the free energies of populations, which are >= 0, finite, few-valued and highest
where the data is sparse.  Here: continuous values (many per quantisation level of the pruned order), ties one ulp
apart, +-0, spans that overflow, subnormals, +-inf, NaN, gradients, anti-density, and free energies that send a whole
cluster's lower neighbours into another one -- through every variant, the sweep forms, the sharded entry points, a
misaligned free-energy array, repeated stats_valid calls, the cross-component pass, host pointers and sessions.
The referee (oracle/dc_oracle.c) compares fe[j] < fe[i] in IEEE arithmetic: NaN is never lower, a NaN frame has no
lower neighbour, -0.0 is not lower than +0.0."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_families
from clustering_amd.synth import gaussian_blobs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FLT_MAX = np.finfo(np.float32).max
FAMILIES = sorted(fe_families.FAMILIES)
FINITE = [f for f in FAMILIES if f not in ("inf", "nan")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


def _supported(variant, n_cols):
    from clustering_amd import capi
    if variant in ("direct", "auto"):
        return True
    if capi.lib.dc_hip_workspace_bytes(64, n_cols, 1) == 0:
        return False
    return variant != "mfma32" or n_cols in (9, 10)


def _radius(D):
    return 0.2 if D <= 10 else float(0.08 * np.sqrt(2.0 * D))


def blobs(n, D, seed):
    c = gaussian_blobs(n, D, seed=seed)
    if n >= 64:
        rng = np.random.default_rng(seed)
        c[rng.integers(0, n, n // 16)] = c[rng.integers(0, n, n // 16)]   # duplicates: ties on d2, lowest index wins
    return c


def family_fe(oracle, c, name, seed=0, pops=None):
    if name in fe_families.NEEDS_POPS and pops is None:
        pops = oracle.populations(c, [_radius(c.shape[1])])[0]
    return fe_families.make(name, c, pops, seed=seed)


def same(got, exp, what):
    """all four outputs (torch tensors or numpy arrays) against the oracle's"""
    g = [t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in got]
    assert (g[0].astype(np.uint32).astype(np.uint64) == exp[0]).all(), (what, "nn_idx")
    assert (g[2].astype(np.uint32).astype(np.uint64) == exp[2]).all(), (what, "hd_idx")
    assert (bits(g[1]) == bits(exp[1])).all(), (what, "nn_d2")
    assert (bits(g[3]) == bits(exp[3])).all(), (what, "hd_d2")


# (n_rows, n_cols): the MFMA widths with the templated direct kernels, the generic direct kernels, the wide sweep;
# rows around a tile of 32, a few thousand (several query groups) and about 20 000 (many cells, many components' tiles)
SHAPES = [(1, 3), (2, 10), (31, 1), (32, 2), (33, 17), (65, 30), (65, 64), (1500, 1), (4097, 3), (4097, 10),
          (2000, 17), (3000, 30), (2500, 64), (20011, 10), (20000, 2), (33, 65), (1200, 65), (700, 100), (2, 401),
          (33, 401), (300, 401)]
VARIANTS = ["direct", "mfma", "pruned", "auto", "mfma32"]


@pytest.mark.parametrize("n_rows,D", SHAPES, ids=[f"{n}x{d}" for n, d in SHAPES])
def test_variants_and_families_against_the_oracle(dens, oracle, n_rows, D):
    """every family through every variant that serves the width, all rows and a row range [lo, hi) (sentinels
    outside it)"""
    import torch
    c = blobs(n_rows, D, seed=n_rows * 7 + D)
    ct = torch.from_numpy(c).cuda()
    pops = oracle.populations(c, [_radius(D)])[0]
    lo, hi = n_rows // 3, n_rows // 3 + max(1, n_rows // 2)
    for fam in FAMILIES:
        fe = family_fe(oracle, c, fam, seed=D, pops=pops)
        fet = torch.from_numpy(fe).cuda()
        exp_full = oracle.nearest_neighbors(c, fe)
        exp_part = oracle.nearest_neighbors(c, fe, lo, hi)
        for variant in VARIANTS:
            if not _supported(variant, D):
                continue
            same(dens.nearest_neighbors_partial(ct, fet, variant=variant), exp_full, (fam, variant, "all rows"))
            same(dens.nearest_neighbors_partial(ct, fet, lo, hi, variant=variant), exp_part, (fam, variant, lo, hi))


_FORMS_CHILD = r"""
import json, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import fe_families
from clustering_amd import density as dens
from clustering_amd.synth import gaussian_blobs
from oracle.oracle import Oracle
oracle = Oracle()
cases, families = json.loads(sys.argv[2]), json.loads(sys.argv[3])
def check(got, exp, what):
    g = [t.cpu().numpy() for t in got]
    assert (g[0].astype(np.uint32).astype(np.uint64) == exp[0]).all(), (what, "nn_idx")
    assert (g[2].astype(np.uint32).astype(np.uint64) == exp[2]).all(), (what, "hd_idx")
    assert (g[1].view(np.uint32) == exp[1].view(np.uint32)).all(), (what, "nn_d2")
    assert (g[3].view(np.uint32) == exp[3].view(np.uint32)).all(), (what, "hd_d2")
for n, d in cases:
    c = gaussian_blobs(n, d, seed=3 * n + d)
    rng = np.random.default_rng(n)
    c[rng.integers(0, n, n // 16)] = c[rng.integers(0, n, n // 16)]
    ct = torch.from_numpy(c).cuda()
    pops = oracle.populations(c, [0.2 if d <= 10 else 0.08 * np.sqrt(2.0 * d)])[0]
    lo, hi = n // 4, n // 4 + n // 3
    for fam in families:
        fe = fe_families.make(fam, c, pops, seed=d)
        fet = torch.from_numpy(fe).cuda()
        exp = oracle.nearest_neighbors(c, fe)
        check(dens.nearest_neighbors_partial(ct, fet, variant="pruned"), exp, (n, d, fam, "all rows"))
        check(dens.nearest_neighbors_partial(ct, fet, lo, hi, variant="pruned"), oracle.nearest_neighbors(c, fe, lo, hi),
              (n, d, fam, "row range"))
        words = None
        for g in range(3):
            w = dens.pack_neighbors(*dens.nearest_neighbors_segment(ct, fet, g, 3))
            words = w if words is None else torch.minimum(words, w)
        check(dens.unpack_neighbors(words), exp, (n, d, fam, "segments"))
print("ok")
"""

FORM_FAMILIES = ["continuous", "ties_ulp", "signed_zero", "inf", "anti_density", "nan"]
FORMS = [({"DC_NN_SHARED": "1"}, [(3000, 24), (2500, 30), (33, 30), (1500, 40)]),
         ({"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "8"}, [(3000, 10), (2000, 17), (4097, 3)]),
         ({"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "16"}, [(3000, 10), (2500, 30)]),
         ({"DC_NN_COOP": "0"}, [(3000, 10), (2500, 30)]),
         ({"DC_WAVES_PER_GROUP": "1"}, [(3000, 10), (2000, 17)]),
         ({"DC_WAVES_PER_GROUP": "4"}, [(3000, 10), (2000, 17)]),
         ({"DC_NN_FE_BITS": "0"}, [(3000, 10), (4097, 3)]),
         ({"DC_NN_FE_BITS": "1"}, [(3000, 10), (2500, 30)]),
         ({"DC_NN_FE_BITS": "16"}, [(3000, 10), (4097, 3)])]


@pytest.mark.parametrize("extra,cases", FORMS, ids=[",".join(f"{k}={v}" for k, v in e.items()) for e, _ in FORMS])
def test_sweep_forms_with_free_energies_of_any_origin(extra, cases):
    """each form of the pruned neighbour sweep in its own process (the switches are read once per process): the
    shared-operand sweep, the cooperative shares, one or four waves per group, 0 / 1 / 16 free-energy bits in the order
    key -- all rows, a row range and three segments against the oracle"""
    r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, ROOT, json.dumps(cases), json.dumps(FORM_FAMILIES)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, **extra))
    assert r.returncode == 0 and "ok" in r.stdout, (extra, r.stderr[-3000:])


@pytest.mark.parametrize("n_rows,D", [(5000, 10), (1000, 30), (37, 2), (3000, 70)])
@pytest.mark.parametrize("fam", ["continuous", "per_cluster", "nan"])
def test_sharded_entry_points(dens, oracle, n_rows, D, fam):
    """the min-merge of nearest_neighbors_segment + pack_neighbors over G segments, and the dense blocks of
    pack_neighbor_block / unpack_neighbor_blocks, against the oracle"""
    import torch
    c = blobs(n_rows, D, seed=11 * n_rows + D)
    ct = torch.from_numpy(c).cuda()
    fe = family_fe(oracle, c, fam, seed=D)
    fet = torch.from_numpy(fe).cuda()
    exp = oracle.nearest_neighbors(c, fe)
    for G in (2, 3, 8):
        words, blocks = None, []
        for g in range(G):
            a, b, cc, d = dens.nearest_neighbors_segment(ct, fet, g, G)
            blocks.append(dens.pack_neighbor_block(ct, a, b, cc, d, g, G))
            w = dens.pack_neighbors(a, b, cc, d)
            words = w if words is None else torch.minimum(words, w)
        same(dens.unpack_neighbors(words.contiguous()), exp, (fam, G, "min-merge"))
        same(dens.unpack_neighbor_blocks(ct, torch.stack(blocks).contiguous(), G), exp, (fam, G, "blocks"))


@pytest.mark.parametrize("n_rows,D", [(4097, 10), (1023, 3), (2001, 30), (37, 17)])
def test_misaligned_free_energies(dens, oracle, n_rows, D):
    """free energies as a contiguous view that starts 4 bytes into a buffer, n_rows not a multiple of 4: the scalar
    path of fe_key_kernel and its tail"""
    import torch
    c = blobs(n_rows, D, seed=5 * n_rows + D)
    ct = torch.from_numpy(c).cuda()
    for fam in ("continuous", "ties_ulp", "signed_zero", "nan"):
        fe = family_fe(oracle, c, fam, seed=D)
        buf = torch.full((n_rows + 8,), -7.0, dtype=torch.float32, device="cuda")
        view = buf[1:n_rows + 1]
        view.copy_(torch.from_numpy(fe))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        exp = oracle.nearest_neighbors(c, fe)
        for variant in ("mfma", "pruned"):
            same(dens.nearest_neighbors_partial(ct, view, variant=variant), exp, (fam, variant))


def test_stats_valid_with_changing_free_energies(dens, oracle):
    """one coordinate array, one populations call, then neighbour calls with stats_valid=True and other free energies
    each time: each equals the oracle for ITS free energies (the claim refreshes the free-energy extremes, header words
    12 / 13, and the order); the finite ones are answered by the pruned sweep, NaN ones by the direct kernels.  A
    constant 3.5 before continuous values below it: a stale minimum of 3.5 would hide every lower neighbour."""
    import torch
    n, D = 6000, 10
    c = blobs(n, D, seed=61)
    ct = torch.from_numpy(c).cuda()
    pops = dens.calculate_populations_partial(ct, [0.2])
    assert (pops.cpu().numpy().astype(np.uint32).astype(np.uint64) == oracle.populations(c, [0.2])).all()
    for k, fam in enumerate(["continuous", "constant_3_5", "continuous", "constant", "nan", "continuous", "ties_ulp",
                             "inf", "gradient", "signed_zero", "continuous"]):
        fe = family_fe(oracle, c, fam, seed=100 + k)
        got = dens.nearest_neighbors_partial(ct, torch.from_numpy(fe).cuda(), stats_valid=True)
        same(got, oracle.nearest_neighbors(c, fe), (k, fam))
        tiles = dens.evaluated_tiles(ct.device)[1]
        if fam == "nan":
            assert tiles == 0, (k, fam, "NaN free energies: the direct kernels answer")
        elif fam in FINITE:
            assert tiles > 0, (k, fam, "the pruned sweep answered")


def _two_clusters(n_half, D, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 1.0, (n_half, D))
    b = rng.normal(0.0, 1.0, (n_half, D))
    a[:, 0] -= 500.0
    b[:, 0] += 500.0
    return np.ascontiguousarray(np.concatenate([a, b]), dtype=np.float32)


def _cross_component_setup(dens, oracle, n_half, D):
    import torch
    c = _two_clusters(n_half, D, seed=n_half + D)
    ct = torch.from_numpy(c).cuda()
    dens.calculate_populations_partial(ct, [0.5], variant="pruned")
    assert dens.components_info(ct)["n_components"] == 2
    fe = family_fe(oracle, c, "per_cluster", seed=D)
    in_a = fe_families.cluster_a(c)
    assert in_a.sum() == n_half and in_a[:n_half].all()
    return c, ct, fe, in_a


def test_cross_component_pass_small(dens, oracle):
    """two clusters far apart, every frame of cluster A with its lower neighbour in cluster B (asserted on the oracle's
    answer): the pruned sweep equals the oracle on all rows"""
    import torch
    c, ct, fe, in_a = _cross_component_setup(dens, oracle, 5000, 10)
    exp = oracle.nearest_neighbors(c, fe)
    assert not in_a[exp[2][in_a].astype(np.int64)].any(), "every frame of A has its lower neighbour in B"
    same(dens.nearest_neighbors_partial(ct, torch.from_numpy(fe).cuda(), variant="pruned"), exp, "pruned")
    same(dens.nearest_neighbors_partial(ct, torch.from_numpy(fe).cuda(), variant="auto"), exp, "auto")


def test_cross_component_pass_many_open_queries(dens, oracle):
    """the same with 2 x 140 000 rows: nn_cross_kernel's one-share branch (>= 1 << 17 open queries).  The open count is
    not visible from Python; it holds by construction: no frame of A is lower than another, so each frame of A has no
    lower-energy incumbent in its own component, and the gap to B's box is at most the distance to any frame of B --
    all 140 000 frames of A are open.  Pruned = direct on every row, = the oracle on three row ranges (one inside A)."""
    import torch
    n_half = 140000
    c, ct, fe, in_a = _cross_component_setup(dens, oracle, n_half, 4)
    fet = torch.from_numpy(fe).cuda()
    got = dens.nearest_neighbors_partial(ct, fet, variant="pruned")
    want = dens.nearest_neighbors_partial(ct, fet, variant="direct")
    for x, y, what in zip(got, want, ("nn_idx", "nn_d2", "hd_idx", "hd_d2")):
        assert bool((x.view(torch.int32) == y.view(torch.int32)).all()), what
    hd = got[2].cpu().numpy().astype(np.int64)
    assert (hd[:n_half] >= n_half).all() and (hd[:n_half] < 2 * n_half).all(), "A's lower neighbours are all in B"
    g = [t.cpu().numpy() for t in got]
    for lo, hi in ((1000, 1600), (n_half - 300, n_half + 300), (2 * n_half - 600, 2 * n_half)):
        exp = oracle.nearest_neighbors(c, fe, lo, hi)
        part = [a[lo:hi] for a in g]
        same(part, [e[lo:hi] for e in exp], (lo, hi))
        assert not in_a[exp[2][lo:hi][in_a[lo:hi]].astype(np.int64)].any()


def test_host_pointer_entry_point(oracle):
    """dc_hip_nearest_neighbors with HOST pointers"""
    from clustering_amd import capi
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for n, D in ((2000, 10), (777, 30)):
        c = blobs(n, D, seed=n + D)
        for fam in ("continuous", "nan", "inf"):
            fe = family_fe(oracle, c, fam, seed=D)
            out = [np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.float32)]
            capi.check(capi.lib.dc_hip_nearest_neighbors(vp(c), n, D, vp(fe), 0, n, 0, *[vp(a) for a in out]))
            same(out, oracle.nearest_neighbors(c, fe), (n, D, fam))


def test_session_set_free_energies(oracle):
    """dc_hip_session_set_free_energies (-D re-use on resident coordinates): all four outputs and sigma2"""
    from clustering_amd import density
    for n, D in ((3000, 10), (1500, 30)):
        c = blobs(n, D, seed=2 * n + D)
        with density.Session(c) as s:
            s.populations([_radius(D)])
            for k, fam in enumerate(("continuous", "inf", "nan", "continuous")):
                fe = family_fe(oracle, c, fam, seed=D + k)
                s.set_free_energies(fe)
                got = s.nearest_neighbors()
                exp = oracle.nearest_neighbors(c, fe)
                same(got[:4], exp, (n, D, fam))
                assert got[4] == oracle.sigma2(exp[1]), (n, D, fam)
