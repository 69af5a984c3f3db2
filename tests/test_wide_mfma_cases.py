"""CPU: the case generators of the wide matrix-core sweeps' tests (tests/wideref.py) really hold what the GPU tests
(tests/test_gpu_wide_mfma.py) rely on: pairs exactly on a radius and one ulp to either side, equal-distance neighbours
and duplicates, and blob data whose pairs almost all lie clear of the kernel's band."""
import numpy as np
import pytest

import refmath
import wideref

F32 = np.float32


@pytest.mark.parametrize("n_rows,n_cols", [(97, 65), (1500, 128), (300, 256)])
def test_boundary_case_holds_pairs_on_the_radius_and_one_ulp_to_either_side(oracle, n_rows, n_cols):
    c, r, groups = wideref.boundary_case(n_rows, n_cols)
    r2 = F32(F32(r) * F32(r))
    assert len(groups) == 3 and len({x for g in groups for x in g}) == 12
    for a, b, cc, d in groups:
        for order in ("sse2", "avx", "fma"):
            from oracle.oracle import Oracle
            o = Oracle(order=order)
            assert o.dist2(c[a], c[b]) == r2 and o.dist2(c[b], c[a]) == r2, (order, a, b)
            assert o.dist2(c[a], c[cc]) == np.nextafter(r2, F32(np.inf)), (order, a, cc)
            assert o.dist2(c[a], c[d]) == np.nextafter(r2, F32(0)), (order, a, d)
    # the strict comparison: the pair on the radius does not count, the one an ulp inside does
    pops = oracle.populations(c, [r])[0]
    a, b, cc, d = groups[0]
    near = refmath.d2_matrix(c[[a, b, cc, d]])
    assert bool(near[0, 3] < r2) and not bool(near[0, 1] < r2) and not bool(near[0, 2] < r2)
    assert pops[a] >= 2
    if n_rows >= 128:
        assert len({x // 32 for x in groups[0]}) >= 3, "rows of a group in different tiles"


@pytest.mark.parametrize("n_rows,n_cols", [(97, 80), (1500, 129)])
def test_ties_case_holds_equal_distance_neighbours_and_duplicates(oracle, n_rows, n_cols):
    c, stars, dups = wideref.ties_case(n_rows, n_cols)
    d2 = refmath.d2_matrix(c) if n_rows <= 200 else None
    fe = oracle.free_energies(oracle.populations(c, [1.0])[0])
    nn_idx, nn_d2, _, _ = oracle.nearest_neighbors(c, fe)
    for q, ring in stars:
        dist = [oracle.dist2(c[q], c[r]) for r in ring]
        assert len(set(float(x) for x in dist)) == 1 and dist[0] == F32(2.0 ** -12), (q, dist)
        assert int(nn_idx[q]) == min(ring) and nn_d2[q] == dist[0], "the lowest index of the tied ring wins"
        assert min(ring) != ring[0] or sorted(ring) != ring, "the ring is not met in index order"
        if d2 is not None:
            row = d2[q].copy()
            row[q] = np.inf
            assert int((row == row.min()).sum()) == 4
    for copy, orig in dups:
        assert (c[copy] == c[orig]).all() and oracle.dist2(c[copy], c[orig]) == 0
        assert nn_d2[copy] == 0 and nn_d2[orig] == 0
        assert int(nn_idx[max(copy, orig)]) == min(copy, orig)


@pytest.mark.parametrize("n_cols", [65, 100, 128, 256])
def test_blob_case_keeps_its_pairs_clear_of_the_band(n_cols):
    """the share of pairs within 2 eps of a threshold (radii at the 25 % and 5 % quantiles of d2) stays under 1 %, eps
    being the band the kernel uses"""
    c = wideref.blobs(1500, n_cols)
    x = c.astype(np.float64)
    g = (x * x).sum(axis=1)
    d2 = np.maximum(g[:, None] + g[None, :] - 2.0 * (x @ x.T), 0.0)
    off = d2[~np.eye(len(c), dtype=bool)]
    for q in (0.25, 0.05):
        r2 = float(np.quantile(off, q))
        e = wideref.eps(n_cols, c, r2)
        share = float((np.abs(off - r2) < 2.0 * e).mean())
        print(f"D={n_cols} quantile {q}: r2={r2:.4f} eps={e:.3e} share within 2 eps = {100 * share:.4f} %")
        assert e > 0 and share < 0.01, (n_cols, q, share)
