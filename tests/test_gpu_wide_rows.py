"""Rows wider than 400 columns (dc_wide.hip, the column-chunked exact sweep): populations, free energies, neighbours, the
radius graph, sessions and the command line against the CPU oracle of the library's summation order
(oracle.oracle.Oracle / Probe with order=capi.CANON_ORDER), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from clustering_amd.synth import gaussian_blobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "clustering_amd", "bin", "clustering")
ALL_ONES = np.iinfo(np.uint64).max
# every residue mod 8 above the seam, both tails, and widths of several chunks
WIDTHS = [401, 402, 403, 404, 405, 406, 407, 408, 409, 415, 416, 512, 1000, 1031]


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


@pytest.fixture(scope="module")
def order():
    from clustering_amd import capi
    return capi.CANON_ORDER


@pytest.fixture(scope="module")
def canon_probe(order):
    from oracle.oracle import Probe, build
    build()
    return Probe(order=order)


@pytest.fixture(scope="module")
def canon_oracle(order):
    from oracle.oracle import Oracle, build
    build()
    return Oracle(order=order)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


def radius(D, f=1.0):
    return float(np.float32(0.08 * np.sqrt(2.0 * D) * f))


def blobs_with_duplicates(n, D, seed):
    c = gaussian_blobs(n, D, seed=seed)
    k = max(1, n // 9)
    if n >= 3 * k + k:
        c[:k] = c[n // 3: n // 3 + k]   # duplicated rows: ties at distance 0 go to the lowest index
    return c


def check_density(dens, o, c, radii, i_from=0, i_to=None):
    """pops / fe / nn (and nn_hd) of rows [i_from, i_to) equal the oracle's, bit for bit"""
    import torch
    n = c.shape[0]
    i_to = n if i_to is None else i_to
    ct = torch.from_numpy(c).cuda()
    want = o.populations(c, radii)
    pops = dens.calculate_populations_partial(ct, radii, i_from, i_to, variant="direct")
    assert (u64(pops)[:, i_from:i_to] == want[:, i_from:i_to]).all(), "pops"
    assert (u64(pops)[:, :i_from] == 0).all() and (u64(pops)[:, i_to:] == 0).all(), "rows outside the range"
    fe_want = o.free_energies(want[0])
    fe = dens.calculate_free_energies(torch.from_numpy(want[0].astype(np.int32)).cuda())
    assert (bits(fe.cpu().numpy()) == bits(fe_want)).all(), "fe"
    exp = o.nearest_neighbors(c, fe_want)
    got = [t.cpu().numpy() for t in dens.nearest_neighbors_partial(ct, fe, i_from, i_to, variant="direct")]
    sl = slice(i_from, i_to)
    assert (got[0].astype(np.uint32).astype(np.uint64)[sl] == exp[0][sl]).all(), "nn idx"
    assert (got[2].astype(np.uint32).astype(np.uint64)[sl] == exp[2][sl]).all(), "nn_hd idx"
    assert (bits(got[1])[sl] == bits(exp[1])[sl]).all(), "nn d2"
    assert (bits(got[3])[sl] == bits(exp[3])[sl]).all(), "nn_hd d2"
    return want, fe_want, exp


@pytest.mark.parametrize("D", WIDTHS)
def test_parity_every_width(dens, canon_oracle, D):
    c = blobs_with_duplicates(300, D, seed=1000 + D)
    r = radius(D)
    check_density(dens, canon_oracle, c, [r])
    check_density(dens, canon_oracle, c, [r * 0.9, r, r * 1.2])


@pytest.mark.parametrize("D", [401, 408, 1031])
def test_nine_radii_two_launches(dens, canon_oracle, D):
    c = blobs_with_duplicates(600, D, seed=1100 + D)
    radii = [radius(D, f) for f in (0.6, 0.7, 0.8, 0.9, 1.0, 1.1, 1.2, 1.4, 3.0)]
    check_density(dens, canon_oracle, c, radii)


@pytest.mark.parametrize("n", [1, 2, 31, 63, 64, 65, 257, 1500])
def test_ragged_sizes(dens, canon_oracle, n):
    D = 403 if n != 1500 else 1000
    check_density(dens, canon_oracle, blobs_with_duplicates(n, D, seed=1200 + n), [radius(D)])


@pytest.mark.parametrize("i_from,i_to", [(0, 0), (7, 7), (0, 1), (5, 70), (63, 65), (200, 257), (1, 257)])
def test_row_ranges(dens, canon_oracle, i_from, i_to):
    c = blobs_with_duplicates(257, 405, seed=1300)
    check_density(dens, canon_oracle, c, [radius(405)], i_from, i_to)


def test_segments_and_neighbour_blocks(dens, canon_oracle):
    import torch
    D, n = 410, 900
    c = blobs_with_duplicates(n, D, seed=1400)
    ct = torch.from_numpy(c).cuda()
    radii = [radius(D), radius(D, 1.2)]
    want = canon_oracle.populations(c, radii)
    acc = None
    for s in range(3):
        p = dens.calculate_populations_segment(ct, radii, s, 3)
        acc = p.clone() if acc is None else acc + p
    assert (u64(acc) == want).all()
    fe_want = canon_oracle.free_energies(want[0])
    fe = torch.from_numpy(fe_want).cuda()
    exp = canon_oracle.nearest_neighbors(c, fe_want)
    rows = dens.neighbor_block_rows(n, D, 3)
    blocks = torch.empty((3, 4, rows), dtype=torch.int32, device=ct.device)
    words = None
    for s in range(3):
        nn = dens.nearest_neighbors_segment(ct, fe, s, 3)
        w = dens.pack_neighbors(*nn)
        words = w if words is None else torch.minimum(words, w)
        dens.pack_neighbor_block(ct, *nn, s, 3, out=blocks[s])
    for got in (dens.unpack_neighbors(words), dens.unpack_neighbor_blocks(ct, blocks, 3)):
        got = [t.cpu().numpy() for t in got]
        assert (got[0].astype(np.uint32).astype(np.uint64) == exp[0]).all()
        assert (got[2].astype(np.uint32).astype(np.uint64) == exp[2]).all()
        assert (bits(got[1]) == bits(exp[1])).all() and (bits(got[3]) == bits(exp[3])).all()


def test_non_finite_cells(dens, canon_oracle):
    D = 407
    c = blobs_with_duplicates(500, D, seed=1500)
    c[17, 3] = np.inf
    c[300, 0] = np.nan
    c[301, D - 1] = -np.inf      # (in the tail columns)
    c[302, D - 5] = np.nan
    want, _, exp = check_density(dens, canon_oracle, c, [radius(D), float("inf")])
    bad = [17, 300, 301, 302]
    assert (want[:, bad] == 1).all()
    assert not np.isin(exp[0], bad).any()


@pytest.mark.parametrize("r", [0.0, float("inf"), float("nan")])
def test_edge_radii(dens, canon_oracle, r):
    c = blobs_with_duplicates(200, 409, seed=1600)
    check_density(dens, canon_oracle, c, [r, radius(409)])


@pytest.mark.parametrize("scale,offset", [(1e-17, 0.0), (1e17, 0.0), (1.0, 1000.0)])
def test_scale_and_offset(dens, canon_oracle, scale, offset):
    D = 404
    c = (blobs_with_duplicates(300, D, seed=1700) * np.float32(scale) + np.float32(offset)).astype(np.float32)
    check_density(dens, canon_oracle, c, [radius(D) * scale, radius(D) * scale * 1.5])


def test_very_wide_few_rows(dens, canon_oracle):
    rng = np.random.default_rng(1800)
    D = 1_000_003
    c = rng.standard_normal((5, D), dtype=np.float32) * np.float32(0.01)
    c[3] = c[1]
    c[4] = c[0] + np.float32(1e-4)
    d2 = float(np.float32(0.01) ** 2 * 2 * D)
    check_density(dens, canon_oracle, np.ascontiguousarray(c), [float(np.sqrt(d2) * 0.5), float(np.sqrt(d2) * 1.5)])


def brute_pairs(probe, c, r2):
    d2 = probe.pairwise_d2(c)
    ii, jj = np.nonzero(np.triu(d2 < np.float32(r2), k=1))
    return np.stack([ii, jj], axis=1).astype(np.int64)


def keys(pairs, n):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.minimum(p[:, 0], p[:, 1]) * n + np.maximum(p[:, 0], p[:, 1])


def degrees(pairs, n):
    deg = np.ones(n, dtype=np.int64)
    np.add.at(deg, pairs[:, 0], 1)
    np.add.at(deg, pairs[:, 1], 1)
    return deg


def raw_pairs(dens, ct, r2, capacity):
    import torch
    from clustering_amd import capi
    n, d = ct.shape
    pops = torch.zeros(n, dtype=torch.int32, device=ct.device)
    count = torch.zeros(1, dtype=torch.int64, device=ct.device)
    pairs = torch.full((capacity, 2), -1, dtype=torch.int32, device=ct.device) if capacity else None
    with torch.cuda.device(ct.device):
        rc = capi.lib.dc_hip_radius_pairs_dev(dens._dev(ct), n, d, float(r2), dens._dev(pops),
                                              dens._dev(pairs) if pairs is not None else None, capacity,
                                              dens._dev(count), None, 0, dens._stream_ptr())
    capi.check(rc, "dc_hip_radius_pairs_dev")
    torch.cuda.synchronize()
    return int(count.item()), (pairs.cpu().numpy() if pairs is not None else None), pops.cpu().numpy()


@pytest.mark.parametrize("n,D", [(1500, 401), (700, 1000), (300, 1031)])
def test_radius_pairs(dens, canon_probe, canon_oracle, n, D):
    import torch
    c = blobs_with_duplicates(n, D, seed=1900 + D)
    c[5, 2] = np.nan
    r = radius(D)
    r2 = np.float32(np.float32(r) * np.float32(r))
    ct = torch.from_numpy(c).cuda()
    pairs, pops = dens.radius_pairs(ct, r2)
    got = keys(pairs.cpu().numpy(), n)
    want = brute_pairs(canon_probe, c, r2)
    assert len(want) > 0
    assert len(np.unique(got)) == len(got)
    assert np.array_equal(np.sort(got), keys(want, n))
    assert (pops.cpu().numpy().astype(np.int64) == degrees(want, n)).all()
    assert (pops.cpu().numpy().astype(np.uint64) == canon_oracle.populations(c, [r])[0]).all()
    count, _, pops_c = raw_pairs(dens, ct, r2, 0)
    assert count == len(want) and (pops_c.astype(np.int64) == degrees(want, n)).all()
    short = max(1, len(want) // 3)
    count, part, _ = raw_pairs(dens, ct, r2, short)
    assert count == len(want)
    assert np.isin(keys(part, n), keys(want, n)).all() and len(np.unique(keys(part, n))) == short


def min_edge_brute(pairs, comp, rank, n):
    want = np.full(n, ALL_ONES, dtype=np.uint64)
    a, b = pairs[:, 0], pairs[:, 1]
    cross = comp[a] != comp[b]
    a, b = a[cross], b[cross]
    hi = np.maximum(rank[a], rank[b]).astype(np.uint64)
    lo = np.minimum(rank[a], rank[b]).astype(np.uint64)
    key = (hi << np.uint64(32)) | lo
    np.minimum.at(want, comp[a], key)
    np.minimum.at(want, comp[b], key)
    return want


def test_min_edge_round_and_segments(dens, canon_probe):
    import torch
    n, D = 1500, 406
    c = blobs_with_duplicates(n, D, seed=2000)
    r = radius(D)
    r2 = np.float32(np.float32(r) * np.float32(r))
    rng = np.random.default_rng(D)
    rank = rng.permutation(n).astype(np.int32)
    label = rng.integers(0, 40, n)
    comp = np.empty(n, dtype=np.int32)
    for lab in np.unique(label):
        members = np.nonzero(label == lab)[0]
        comp[members] = members.min()
    ct, compt, rankt = torch.from_numpy(c).cuda(), torch.from_numpy(comp).cuda(), torch.from_numpy(rank).cuda()
    best, pops = dens.radius_min_edge(ct, r2, compt, rankt)
    pairs = brute_pairs(canon_probe, c, r2)
    want = min_edge_brute(pairs, comp, rank, n)
    got = best.cpu().numpy().view(np.uint64)
    assert (want != ALL_ONES).sum() > 10
    assert (got == want).all()
    assert (pops.cpu().numpy().astype(np.int64) == degrees(pairs, n)).all()
    acc_b = np.full(n, ALL_ONES, dtype=np.uint64)
    acc_p = np.zeros(n, dtype=np.int64)
    for g in range(3):
        b, p = dens.radius_min_edge(ct, r2, compt, rankt, g, 3)
        acc_b = np.minimum(acc_b, b.cpu().numpy().view(np.uint64))
        acc_p += p.cpu().numpy().astype(np.int64)
    assert (acc_b == got).all() and (acc_p == degrees(pairs, n)).all()


def components(n, pairs):
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)])


def test_radius_forest_and_session(dens, canon_probe, canon_oracle):
    n, D = 1200, 600
    c = blobs_with_duplicates(n, D, seed=2100)
    r = radius(D)
    r2 = np.float32(np.float32(r) * np.float32(r))
    rank = np.random.default_rng(2100).permutation(n).astype(np.uint32)
    edges, rounds = dens.radius_forest(c, r2, rank)
    all_pairs = brute_pairs(canon_probe, c, r2)
    assert np.isin(keys(edges, n), keys(all_pairs, n)).all()
    assert len(edges) == n - len(np.unique(components(n, all_pairs))) and len(edges) > 0
    w_all = np.maximum(rank[all_pairs[:, 0]], rank[all_pairs[:, 1]])
    w_for = np.maximum(rank[edges[:, 0]], rank[edges[:, 1]])
    for t in [0, n // 7, n // 3, n // 2, (3 * n) // 4, n]:
        assert (components(n, all_pairs[w_all < t]) == components(n, edges[w_for < t])).all(), t
    assert 1 <= rounds <= 26
    # a resident session gives what the call-by-call path gives
    radii = [r, r * 1.3]
    want = canon_oracle.populations(c, radii)
    fe_want = canon_oracle.free_energies(want[0])
    exp = canon_oracle.nearest_neighbors(c, fe_want)
    with dens.Session(c, n_devices=1) as s:
        pops = s.populations(radii)
        fe = s.free_energies(0)
        nn = s.nearest_neighbors()
        e_s, _ = s.radius_forest(r2, rank)
    pops = np.asarray(pops.cpu() if hasattr(pops, "cpu") else pops)
    assert (pops.astype(np.uint32).astype(np.uint64) == want).all()
    fe = np.asarray(fe.cpu() if hasattr(fe, "cpu") else fe)
    assert (bits(fe) == bits(fe_want)).all()
    nn = [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in nn]
    assert (nn[0].astype(np.uint32).astype(np.uint64) == exp[0]).all()
    assert (nn[2].astype(np.uint32).astype(np.uint64) == exp[2]).all()
    assert (bits(nn[1]) == bits(exp[1])).all() and (bits(nn[3]) == bits(exp[3])).all()
    assert np.array_equal(np.sort(keys(e_s, n)), np.sort(keys(edges, n)))


def data_lines(path):
    return [l for l in open(path).read().splitlines() if l and not l.startswith("#")]


def wide_cli_data(D, n=1500, seed=2200):
    c = gaussian_blobs(n, D, seed=seed)
    c[:, :2] *= np.float32(40.0)   # (blob centres apart: at this width the spread within a blob swamps them)
    return c


@pytest.mark.parametrize("fmt", ["npy", "text"])
def test_cli_wide_rows(tmp_path, fmt):
    from oracle.oracle import Oracle, ScreeningOracle, build
    build()
    o = Oracle()   # (the command line binds the default-order library)
    D = 1000
    c = wide_cli_data(D)
    if fmt == "npy":
        f = tmp_path / "coords.npy"
        np.save(f, c)
    else:
        f = tmp_path / "coords"
        np.savetxt(f, c, fmt="%.9g")
        c = np.loadtxt(f, dtype=np.float64, ndmin=2).astype(np.float32)
    rad = float("%.6f" % radius(D))
    r = subprocess.run([CLI, "density", "-f", str(f), "-r", "%.6f" % rad, "-p", str(tmp_path / "pop"),
                        "-d", str(tmp_path / "fe"), "-b", str(tmp_path / "nn"), "-v"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout
    pops = o.populations(c, [rad])[0]
    fe = o.free_energies(pops)
    nn = o.nearest_neighbors(c, fe)
    assert data_lines(tmp_path / "pop") == [str(int(p)) for p in pops]
    assert data_lines(tmp_path / "fe") == ["%e" % float(np.float32(v)) for v in fe]
    g = lambda x: "%g" % float(np.float32(x))
    assert data_lines(tmp_path / "nn") == ["%d %s %d %s" % (nn[0][i], g(nn[1][i]), nn[2][i], g(nn[3][i]))
                                           for i in range(len(c))]
    # -R: several radii in one run
    radii = ["%.6f" % rad, "%.6f" % (rad * 1.2)]
    r = subprocess.run([CLI, "density", "-f", str(f), "-R", *radii, "-p", str(tmp_path / "popR")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout
    pops_r = o.populations(c, [float(x) for x in radii])
    for k, x in enumerate(radii):
        assert data_lines(str(tmp_path / "popR") + "_%f" % np.float32(x)) == [str(int(p)) for p in pops_r[k]], x
    # -T (forest, then the full graph) and -i against the quadratic restatement
    so = ScreeningOracle()
    for full_graph in (False, True):
        out = tmp_path / ("clust%d" % full_graph)
        r = subprocess.run([CLI, "density", "-f", str(f), "-r", "%.6f" % rad, "-T", "0.5", "1.0", "3.0", "-o", str(out)],
                           capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, DC_SCREENING_FULL_GRAPH="1" if full_graph else "0"))
        assert r.returncode == 0, r.stderr + r.stdout
        clustering = None
        for t in (0.5, 1.5, 2.5):
            clustering = so.screening(fe, nn[1], np.float32(t), c, clustering)
            assert data_lines(str(out) + ".%0.2f" % t) == [str(int(v)) for v in clustering], (full_graph, t)
        assert clustering.max() >= 2
    # -i: an initial clustering, the low-density frames assigned along nn_hd
    initial = so.screening(fe, nn[1], np.float32(1.0), c)
    (tmp_path / "initial").write_text("# initial states\n" + "\n".join(str(int(v)) for v in initial) + "\n")
    r = subprocess.run([CLI, "density", "-f", str(f), "-r", "%.6f" % rad, "-i", str(tmp_path / "initial"),
                        "-o", str(tmp_path / "micro")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr + r.stdout
    want = so.sorted_names(so.assign_low_density(initial, nn[2], fe))
    assert data_lines(tmp_path / "micro") == [str(int(v)) for v in want]


def test_workspace_and_matrix_core_refusals(dens):
    import torch
    from clustering_amd import capi
    assert capi.lib.dc_hip_workspace_bytes(64, 401, 1) == 0
    ct = torch.from_numpy(gaussian_blobs(64, 401, seed=2300)).cuda()
    for v in ("mfma", "pruned", "mfma32"):
        with pytest.raises(RuntimeError):
            dens.calculate_populations_partial(ct, [1.0], variant=v)
    for v in ("auto", "direct"):
        assert dens.calculate_populations_partial(ct, [1.0], variant=v).shape == (1, 64)
