"""The radius graph (dc_hip_radius_pairs_dev, dc_hip_radius_min_edge[_segment]_dev, the forest built on them) for rows
wider than the matrix-core sweep's 64 columns and for coordinates with inf / NaN, served by the direct kernels of
dc_direct.hip (graph_direct_kernel / graph_generic_kernel) -- against brute force over the reference's own pairwise
loop (oracle.oracle.Probe, built with the reference's flags for the summation order of the library under test), and
the command line's screening (-T) against the quadratic restatement (oracle/screening_oracle.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from clustering_amd.synth import gaussian_blobs
from graphref import ALL_ONES, brute_pairs, components, degrees, keys, min_edge_brute, raw_pairs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "clustering_amd", "bin", "clustering")


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


def radius2(D):
    """a radius around the typical within-blob distance (test_parity_generic_dims) and its fl32 square"""
    r = np.float32(0.2) if D <= 10 else np.float32(0.08 * np.sqrt(2.0 * D))
    return r, np.float32(r * r)


def with_non_finite(c):
    c = c.copy()
    D = c.shape[1]
    c[17, 3 % D] = np.inf
    c[400, 0] = np.nan
    c[401, D - 1] = -np.inf
    return c


def check_pair_list(dens, canon_probe, canon_oracle, c, r, r2):
    import torch
    n = c.shape[0]
    ct = torch.from_numpy(c).cuda()
    pairs, pops = dens.radius_pairs(ct, r2)
    got = keys(pairs.cpu().numpy(), n)
    want_pairs = brute_pairs(canon_probe, c, r2)
    assert len(want_pairs) > 0, "the case has no pairs"
    assert len(np.unique(got)) == len(got), "a pair was listed twice"
    assert np.array_equal(np.sort(got), keys(want_pairs, n))
    assert (pairs[:, 0] != pairs[:, 1]).all().item()
    pops = pops.cpu().numpy().astype(np.int64)
    assert (pops == degrees(want_pairs, n)).all()
    assert (pops.astype(np.uint64) == canon_oracle.populations(c, [r])[0]).all()
    # counting only, and a buffer too short for the list: the full count either way, never ~0
    count, _, pops_c = raw_pairs(dens, ct, r2, 0)
    assert count == len(want_pairs)
    assert (pops_c.astype(np.int64) == pops).all()
    short = max(1, len(want_pairs) // 3)
    count, part, _ = raw_pairs(dens, ct, r2, short)
    assert count == len(want_pairs)
    assert np.isin(keys(part, n), keys(want_pairs, n)).all() and len(np.unique(keys(part, n))) == short
    return want_pairs


@pytest.mark.parametrize("n_rows,n_cols", [(1500, 65), (1200, 100), (700, 400)])
def test_radius_pairs_wide_rows(dens, canon_probe, canon_oracle, n_rows, n_cols):
    from clustering_amd import capi
    assert capi.lib.dc_hip_workspace_bytes(n_rows, n_cols, 1) == 0   # (no workspace is passed)
    c = gaussian_blobs(n_rows, n_cols, seed=300 + n_cols)
    r, r2 = radius2(n_cols)
    check_pair_list(dens, canon_probe, canon_oracle, c, r, r2)


@pytest.mark.parametrize("n_cols", [5, 10, 32, 33, 64, 70])
def test_radius_pairs_non_finite_rows(dens, canon_probe, canon_oracle, n_cols):
    """inf / NaN in single cells: such a row has no partners (pop 1), the other rows keep theirs -- on both sides of
    the register-resident / LDS-resident seam (32 / 33) inside the matrix-core width, where only the on-device gate
    sends the data to the direct kernel, and beyond it."""
    c = with_non_finite(gaussian_blobs(900, n_cols, seed=310 + n_cols))
    r, r2 = radius2(n_cols)
    want = check_pair_list(dens, canon_probe, canon_oracle, c, r, r2)
    bad = [17, 400, 401]
    assert not np.isin(want, bad).any()
    import torch
    _, pops = dens.radius_pairs(torch.from_numpy(c).cuda(), r2)
    assert (pops.cpu().numpy()[bad] == 1).all()


@pytest.mark.parametrize("n_cols,non_finite", [(70, False), (10, True)])
def test_min_edge_round_wide_and_flagged(dens, canon_probe, n_cols, non_finite):
    import torch
    n = 1500
    c = gaussian_blobs(n, n_cols, seed=320 + n_cols)
    if non_finite:
        c = with_non_finite(c)
    r, r2 = radius2(n_cols)
    rng = np.random.default_rng(n_cols)
    rank = rng.permutation(n).astype(np.int32)
    label = rng.integers(0, 40, n)
    comp = np.empty(n, dtype=np.int32)           # id of a component = its smallest frame id
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
    # three segments (the reference's row blocks here) merge by unsigned minimum / summation to the whole round
    acc_b = np.full(n, ALL_ONES, dtype=np.uint64)
    acc_p = np.zeros(n, dtype=np.int64)
    for g in range(3):
        b, p = dens.radius_min_edge(ct, r2, compt, rankt, g, 3)
        acc_b = np.minimum(acc_b, b.cpu().numpy().view(np.uint64))
        acc_p += p.cpu().numpy().astype(np.int64)
    assert (acc_b == got).all() and (acc_p == degrees(pairs, n)).all()


@pytest.mark.parametrize("n_rows,n_cols,non_finite", [(1500, 70, False), (1200, 100, False), (2000, 10, True)])
def test_radius_forest_wide_and_flagged(dens, canon_probe, n_rows, n_cols, non_finite):
    """dc_hip_radius_forest: a forest of graph pairs with the graph's connectivity below every rank threshold; the
    resident session's forest (dc_hip_session_radius_forest) is the same."""
    c = gaussian_blobs(n_rows, n_cols, seed=330 + n_cols)
    if non_finite:
        c = with_non_finite(c)
    r, r2 = radius2(n_cols)
    rank = np.random.default_rng(n_rows + n_cols).permutation(n_rows).astype(np.uint32)
    edges, rounds = dens.radius_forest(c, r2, rank)
    all_pairs = brute_pairs(canon_probe, c, r2)
    assert np.isin(keys(edges, n_rows), keys(all_pairs, n_rows)).all()
    full = components(n_rows, all_pairs)
    assert len(edges) == n_rows - len(np.unique(full)), "not a spanning forest"
    assert len(edges) > 0
    w_all = np.maximum(rank[all_pairs[:, 0]], rank[all_pairs[:, 1]])
    w_for = np.maximum(rank[edges[:, 0]], rank[edges[:, 1]]) if len(edges) else np.zeros(0)
    for t in [0, n_rows // 7, n_rows // 3, n_rows // 2, (3 * n_rows) // 4, n_rows]:
        a = components(n_rows, all_pairs[w_all < t])
        b = components(n_rows, edges[w_for < t])
        assert (a == b).all(), f"connectivity differs below rank {t}"
    assert 1 <= rounds <= 26
    with dens.Session(c, n_devices=1) as s:
        e_s, _ = s.radius_forest(r2, rank)
    assert np.array_equal(np.sort(keys(e_s, n_rows)), np.sort(keys(edges, n_rows)))


def data_lines(path):
    return [l for l in open(path).read().splitlines() if l and not l.startswith("#")]


@pytest.mark.parametrize("full_graph", [False, True])
def test_cli_screening_at_70_columns(tmp_path, oracle, full_graph):
    """clustering density -T FROM STEP TO -o on a 70-column file: the forest (default) or the full pair list
    (DC_SCREENING_FULL_GRAPH=1) give, threshold by threshold, the clustering of the quadratic restatement, chained
    through the thresholds like density_clustering.cpp:801-812 (the CLI binds the default-order library)."""
    from oracle.oracle import ScreeningOracle
    so = ScreeningOracle()
    c = gaussian_blobs(2000, 70, seed=470)
    c[:, :2] *= np.float32(4.0)   # (blob centres apart: at 70 columns the spread within a blob is close to their distance)
    np.savetxt(tmp_path / "coords", c, fmt="%.9g")
    c = np.loadtxt(tmp_path / "coords", dtype=np.float64, ndmin=2).astype(np.float32)
    radius = float(np.float32(0.08 * np.sqrt(140.0)))
    r = subprocess.run([CLI, "density", "-f", str(tmp_path / "coords"), "-r", "%.6f" % radius, "-T", "0.5", "0.75", "5.0",
                        "-o", str(tmp_path / "clust"), "-v"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DC_SCREENING_FULL_GRAPH="1" if full_graph else "0"))
    assert r.returncode == 0, r.stderr + r.stdout
    assert ("within the lumping radius" if full_graph else "span the graph") in r.stdout + r.stderr
    pops = oracle.populations(c, [float("%.6f" % radius)])[0]
    fe = oracle.free_energies(pops)
    nn = oracle.nearest_neighbors(c, fe)
    clustering = None
    t, n_files = np.float32(0.5), 0
    t_to, step = np.float32(5.0), np.float32(0.75)
    while t < t_to - step / np.float32(10.0) + step and not (t_to + step / np.float32(10.0) + step < t):
        clustering = so.screening(fe, nn[1], t, c, clustering)
        got = data_lines(str(tmp_path / "clust") + ".%0.2f" % t)
        assert got == [str(int(v)) for v in clustering], f"threshold {t}"
        n_files += 1
        t = np.float32(t + step)
    assert n_files == 7
    assert clustering.max() >= 2          # more than one state at the top threshold


def test_wide_rows_still_need_no_workspace():
    """the direct kernels need no workspace: dc_hip_workspace_bytes stays 0 beyond 64 columns (the matrix-core
    variants stay unsupported there)"""
    from clustering_amd import capi
    assert capi.lib.dc_hip_workspace_bytes(64, 70, 1) == 0
