"""The resident reference of the pruned wide cross sweeps (density.Reference, dc_hip_reference_wide_*) on
the device: every output bit for bit against the unpruned cross sweeps (calculate_populations_against_wide,
nearest_reference_wide) -- batches in sequence on one handle, whatever came before, in every call order, through the
gate, at the edges, inside the pruning bounds formed from the device's own two orders.
Cases and premises: tests/referencewideref.py, tests/test_reference_wide_cases.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crossref
import crosswidennpruneref as nnref
import crosswidepruneref as pr
import crosswideref as cw
import referencewideref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def dens():
    from clustering_amd import density
    return density


@functools.lru_cache(maxsize=None)
def the_probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    """bit for bit: integers as they are, floats by their bits; None only equals None"""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def reference(n_r, n_cols):
    R = ref.reference_rows(n_r, n_cols)
    return R, gpu(R)


def check_batch(dens, h, Q, Rt, radii=None, fe_q=None, fe_r=None, what="", order=("pops", "nn")):
    """stage Q, run the sweeps named in `order`, each against the unpruned call; -> the info tuples of the sweeps"""
    q = gpu(Q)
    h.stage(q)
    infos = []
    for step in order:
        if step == "pops":
            got = h.populations(radii)
            want = dens.calculate_populations_against_wide(q, Rt, radii)
            assert torch.equal(got, want), (what, "populations", len(radii))
        else:
            fq, fr = (None, None) if fe_q is None else (gpu(fe_q), gpu(fe_r))
            got = h.nearest(fq)
            want = dens.nearest_reference_wide(q, Rt, fq, fr)
            for name, a, b in zip(("nn_idx", "nn_d2", "hd_idx", "hd_d2"), got, want):
                assert same(a, b), (what, name, fe_q is not None)
        infos.append(h.info())
    return infos


@pytest.mark.parametrize("n_r,n_cols", ref.REFERENCES)
def test_batches_in_sequence_on_one_handle(dens, n_r, n_cols):
    R, Rt = reference(n_r, n_cols)
    radii9 = cw.radii_for(n_cols, 9)
    if n_r > 2000:
        radii9 = radii9[:8] + [4.0 * radii9[0]]   # one launch of the nine past a list round's worth of survivors
    with dens.Reference(Rt, ref.MAX_BATCH) as h:
        perm_r0 = None
        for k, n_q in enumerate(ref.BATCHES):
            Q = ref.ordinary_batch(R, n_q, seed=40 + k)
            fe_q, fe_r = cw.fe_pair(n_q, n_r, seed=17 + k)
            # every size with 1, 3 and 9 radii, with free energies (new ones per batch) and without
            h.set_free_energies(gpu(fe_r))
            infos = []
            for n_rad, with_fe in ((1, True), (3, False), (9, True)):
                infos += check_batch(dens, h, Q, Rt, radii9[:n_rad], fe_q if with_fe else None, fe_r if with_fe else None,
                                     what=(n_r, n_cols, n_q, n_rad))
            for tiles, mfmas, _, answered, preparations in infos:
                assert answered == 0 and tiles > 0 and mfmas == cw.nm_for(n_cols) * tiles and preparations == 1, (n_q, infos)
            perm_q, perm_r = h.order()
            assert sorted(perm_q.tolist()) == list(range(n_q))
            if perm_r0 is None:
                perm_r0 = perm_r
                assert sorted(perm_r.tolist()) == list(range(n_r))
            assert torch.equal(perm_r, perm_r0), "the reference's order does not move"
        assert h.info()[4] == 1, "the reference was prepared once"


def test_history_does_not_matter(dens):
    R, Rt = reference(1500, 100)
    A, B = ref.headroom_batch(R, 300, seed=51), ref.ordinary_batch(R, 129, seed=52)
    radii = cw.radii_for(100, 3)
    fe_q, fe_r = cw.fe_pair(129, 1500)

    def run_b(h):
        h.stage(gpu(B))
        pops = h.populations(radii)
        ip = h.info()
        nn = h.nearest(gpu(fe_q))
        return pops, nn, ip, h.info()

    with dens.Reference(Rt, 300) as h1, dens.Reference(Rt, 300) as h2:
        for h in (h1, h2):
            h.set_free_energies(gpu(fe_r))
        check_batch(dens, h1, A, Rt, radii, what="A")
        after_a, fresh = run_b(h1), run_b(h2)
        h1.stage(gpu(A))
        again = run_b(h1)
    for other in (fresh, again):
        assert torch.equal(after_a[0], other[0]) and all(same(a, b) for a, b in zip(after_a[1], other[1]))
        assert after_a[2][:2] == other[2][:2] and after_a[3][:2] == other[3][:2], "tiles and mfmas"
    assert after_a[2][2] == again[2][2] and after_a[3][2] == again[3][2], "exact pairs on one handle: the means are fixed"
    assert abs(after_a[2][2] - fresh[2][2]) <= 64, "exact pairs across two opens: a last bit of the means at most"


def test_call_orders_on_one_staged_batch(dens):
    R, Rt = reference(1500, 65)
    Q = ref.ordinary_batch(R, 300, seed=61)
    fe_q, fe_r = cw.fe_pair(300, 1500, seed=3)
    fe_r2 = cw.fe_pair(300, 1500, seed=4)[1]
    r3, r9 = cw.radii_for(65, 3), cw.radii_for(65, 9)
    with dens.Reference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        check_batch(dens, h, Q, Rt, r3, fe_q, fe_r, "pops -> nn", ("pops", "nn"))
        check_batch(dens, h, Q, Rt, r3, fe_q, fe_r, "nn -> pops", ("nn", "pops"))
        q = gpu(Q)
        h.stage(q)
        for radii in (r3, r9[3:], r9, r3[:1]):
            assert torch.equal(h.populations(radii), dens.calculate_populations_against_wide(q, Rt, radii)), "populations twice"
        want = dens.nearest_reference_wide(q, Rt, gpu(fe_q), gpu(fe_r))
        for _ in range(2):
            assert all(same(a, b) for a, b in zip(h.nearest(gpu(fe_q)), want)), "nearest twice"
        assert all(same(a, b) for a, b in zip(h.nearest(), dens.nearest_reference_wide(q, Rt))), "nn only, after the full call"
        assert torch.equal(h.populations(r3), dens.calculate_populations_against_wide(q, Rt, r3)), "populations after the neighbours"
        h.set_free_energies(gpu(fe_r2))
        check_batch(dens, h, Q[:129], Rt, r3, fe_q[:129], fe_r2, "new free energies between two batches")
        assert h.info()[4] == 1


@pytest.mark.parametrize("flaw", ["nan", "inf", "beyond"])
def test_a_flagged_batch_goes_to_the_direct_kernels_and_the_next_one_does_not(dens, flaw):
    R, Rt = reference(1500, 100)
    radii = cw.radii_for(100, 3)
    fe_q, fe_r = cw.fe_pair(300, 1500)
    if flaw == "beyond":
        Q = ref.beyond_batch(R, 300)
    else:
        Q = ref.ordinary_batch(R, 300)
        Q[153, 99] = np.nan if flaw == "nan" else np.inf
    with dens.Reference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        for info in check_batch(dens, h, Q, Rt, radii, fe_q, fe_r, flaw):
            assert info[:4] == (0, 0, 0, 2), info
        for info in check_batch(dens, h, ref.ordinary_batch(R, 300, seed=5), Rt, radii, fe_q, fe_r, "after " + flaw):
            assert info[3] == 0 and info[0] > 0, info


def test_a_batch_inside_the_headroom_and_outside_the_extent_runs_on_the_matrix_cores(dens):
    for n_r, n_cols in ((1500, 65), (1500, 256)):
        R, Rt = reference(n_r, n_cols)
        Q = ref.headroom_batch(R, 300)
        fe_q, fe_r = cw.fe_pair(300, n_r)
        with dens.Reference(Rt, 300) as h:
            h.set_free_energies(gpu(fe_r))
            for info in check_batch(dens, h, Q, Rt, cw.radii_for(n_cols, 3), fe_q, fe_r, "headroom"):
                assert info[3] == 0 and info[0] > 0, info


@pytest.mark.parametrize("flaw", ["nan reference", "inf reference", "big reference"])
def test_a_flagged_reference_opens_and_every_batch_is_answered_by_the_direct_kernels(dens, flaw):
    R = reference(1500, 100)[0]
    _, Rf = cw.flawed_sets(R[:8], R, flaw)
    Rt = gpu(Rf)
    fe_q, fe_r = cw.fe_pair(129, 1500)
    with dens.Reference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        for k in range(2):
            for info in check_batch(dens, h, ref.ordinary_batch(R, 129, seed=70 + k), Rt, cw.radii_for(100, 3), fe_q, fe_r, flaw):
                assert info[:4] == (0, 0, 0, 1), info


@pytest.mark.parametrize("side", ["fe_ref", "fe_query"])
def test_a_nan_free_energy_sends_the_neighbour_sweep_alone_to_the_direct_kernel(dens, side):
    R, Rt = reference(1500, 100)
    Q = ref.ordinary_batch(R, 300)
    fe_q, fe_r = cw.fe_pair(300, 1500)
    (fe_r if side == "fe_ref" else fe_q)[77] = np.nan
    with dens.Reference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        for order in (("pops", "nn"), ("nn", "pops")):
            infos = dict(zip(order, check_batch(dens, h, Q, Rt, cw.radii_for(100, 3), fe_q, fe_r, side, order)))
            assert infos["nn"][:4] == (0, 0, 0, 3), infos
            assert infos["pops"][3] == 0 and infos["pops"][0] > 0, infos
        h.stage(gpu(Q))
        assert all(same(a, b) for a, b in zip(h.nearest(), dens.nearest_reference_wide(gpu(Q), Rt)))
        assert h.info()[3] == 0, "neighbours without free energies read none"
        clean_q, clean_r = cw.fe_pair(300, 1500)
        h.set_free_energies(gpu(clean_r))
        assert check_batch(dens, h, Q, Rt, None, clean_q, clean_r, "clean again", ("nn",))[0][3] == 0


def test_edges_through_the_resident_path(dens):
    cases = []
    Q, R, r, _ = cw.boundary_sets(300, 1500, 100)
    cases.append(("boundary", Q, R, [r]))
    Q, R, *_ = cw.ties_sets(300, 1500, 65)
    cases.append(("ties", Q, R, cw.radii_for(65, 3)))
    Q, R, r, _ = pr.margin_sets()
    cases.append(("margin", Q, R, [r]))
    R1500 = reference(1500, 100)[0]
    cases.append(("reference of 1 row", R1500[5:305], R1500[:1], cw.radii_for(100, 3)))
    cases.append(("reference of 129 rows", ref.ordinary_batch(R1500[:129], 300), R1500[:129], cw.radii_for(100, 3)))
    cases.append(("the batch is the reference", R1500, R1500, cw.radii_for(100, 3)))
    for what, Q, R, radii in cases:
        fe_q, fe_r = cw.fe_pair(len(Q), len(R))
        Rt = gpu(R)
        d2 = crossref.block_d2(the_probe(), Q, R)
        with dens.Reference(Rt, len(Q)) as h:
            h.set_free_energies(gpu(fe_r))
            check_batch(dens, h, Q, Rt, radii, fe_q, fe_r, what)
            # ... and against the probe's canonical d2 of the block, as the tests of the per-call sweeps hold these cases
            assert (crossref.host(h.populations(radii)) == crossref.expect_pops(d2, radii)).all(), (what, "probe, populations")
            crossref.same_nn(h.nearest(gpu(fe_q)), crossref.expect_nn(d2, fe_q, fe_r), what + ", probe")
            check_batch(dens, h, Q, Rt, radii, None, None, what + ", nn only", ("nn",))
            crossref.same_nn(h.nearest(), crossref.expect_nn(d2), what + ", probe, nn only")


def test_the_sweeps_stay_inside_the_pruning_bounds_of_the_devices_own_orders(dens):
    Q, R, fe_q, fe_r = ref.prune_case()
    n_cols, radii = Q.shape[1], pr.radii_for(Q.shape[1], 3)
    Rt = gpu(R)
    with dens.Reference(Rt, len(Q)) as h:
        h.set_free_energies(gpu(fe_r))
        pops_info, nn_info = check_batch(dens, h, Q, Rt, radii, fe_q, fe_r, "pruning")
        perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in h.order())
    lo, hi = pr.tile_bounds(Q, R, perm_q, perm_r, radii)
    g = pr.gaps(Q, R, perm_q, perm_r)
    print(f"populations: tiles {pops_info[0]} in [{lo}, {hi}] of {16 * g.size}")
    assert lo <= pops_info[0] <= hi and hi <= 16 * g.size * 2 // 3, "the pruning check; a third of the block pairs left out"
    lo, hi = nnref.tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)
    print(f"neighbours: tiles {nn_info[0]} in [{lo}, {hi}] of {16 * g.size}")
    assert lo <= nn_info[0] <= hi and hi <= 16 * g.size * 2 // 3


@pytest.mark.parametrize("n_cols", [65, 256])
def test_the_exact_path_takes_the_pairs_of_the_resident_window(dens, n_cols):
    """`exact_pairs` against the float64 count of pairs in the resident window -- |d2 - r^2| < eps, eps from
    test_wide_model --band with M_res = 4 M_ref, the pairs of the surviving block pairs, added over the radii -- from both
    sides.  The device parks a pair when its ACCUMULATOR lies in the window, the float64 count asks the same of S d2: the
    two differ only in pairs within the realised accumulator error of the window's edge.  That error is estimated from the
    number formats (referencewideref.realised_error_share: 2 - 4 % of eps at these shapes, plus 0.1 % for the rounding
    margin of the window arithmetic), so
        #{|d2 - r^2| < (1 - f) eps}  <=  exact_pairs  <=  #{|d2 - r^2| < (1 + f) eps},
    both counted in float64.  A band formed from M_ref instead (about a quarter of the pairs) or one twice too wide fails
    it.  The bound that needs no estimate -- every parked pair has |d2 - r^2| < 2 eps, since the accumulator is within eps
    of S d2 -- is asserted beside it."""
    Q, R = pr.split_sets(1500, 1500, n_cols)
    radii, Rt, q = pr.radii_for(n_cols, 3), gpu(R), gpu(Q)
    with dens.Reference(Rt, len(Q)) as h:
        h.stage(q)
        assert torch.equal(h.populations(radii), dens.calculate_populations_against_wide(q, Rt, radii))
        tiles, _, exact, answered, _ = h.info()
        perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in h.order())
    f = ref.realised_error_share(n_cols, R, radii) + 1e-3
    assert 0.0 < f < 0.1, "the estimate leaves a check that can tell a wrong band"
    twice, _ = ref.window_pairs(n_cols, Q, R, perm_q, perm_r, radii, widen=2.002)
    inside, _ = ref.window_pairs(n_cols, Q, R, perm_q, perm_r, radii)
    lower, _ = ref.window_pairs(n_cols, Q, R, perm_q, perm_r, radii, widen=1.0 - f)
    upper, _ = ref.window_pairs(n_cols, Q, R, perm_q, perm_r, radii, widen=1.0 + f)
    print(f"D={n_cols}: {exact} exact pairs of {1024 * tiles} evaluated = {100.0 * exact / (1024 * tiles):.4f} %; float64 count in "
          f"the window {inside}, at (1 -/+ {f:.4f}) of it {lower} / {upper}, at twice the window {twice}")
    assert answered == 0 and tiles > 0
    assert lower <= exact <= upper, (lower, exact, upper)
    assert exact <= twice


def test_reference_assign_equals_assign_frames_wide_pruned(dens):
    R, Rt = reference(1500, 100)
    Q = np.concatenate([ref.ordinary_batch(R, 2000, seed=81), ref.headroom_batch(R, 500, seed=82)])
    states = (np.arange(1500) % 7).astype(np.int32)
    radius = cw.radii_for(100, 1)[0]
    want = dens.assign_frames_wide_pruned(gpu(Q), Rt, radius, states, pruned_neighbours=True)
    with dens.Reference(Rt, 1000, radius=radius, ref_states=states) as h:
        got = h.assign(gpu(Q))
        none = h.assign(gpu(Q[:0]))
        assert h.info()[4] == 1
    want_none = dens.assign_frames_wide_pruned(gpu(Q[:0]), Rt, radius, states, pruned_neighbours=True)
    for g, w in ((got, want), (none, want_none)):
        assert set(g) == set(w)
        for key in w:
            if key == "max_pop":
                assert g[key] == w[key]
            else:
                assert same(g[key], w[key]), key
    assert none["states"].shape == (0,) and none["nn_idx"].shape == (0,), "no rows: the same dict, empty"
    # what the constructor can refuse it refuses before it opens a handle or allocates
    for kwargs in ({"radius": radius}, {"ref_states": states}, {"radius": radius, "ref_states": states[:-1]}):
        with pytest.raises(ValueError):
            dens.Reference(Rt, 1000, **kwargs)
    with pytest.raises(ValueError):
        dens.Reference(Rt, 0)


def test_refusals_of_a_handle(dens):
    from clustering_amd import capi
    R, Rt = reference(1500, 100)
    Q = gpu(ref.ordinary_batch(R, 300))
    with dens.Reference(Rt, 200) as h:
        for call, words in ((lambda: h.populations([1.0]), None), (lambda: h.nearest(), None)):
            with pytest.raises(ValueError):
                call()
        for fn, args in (("dc_hip_reference_wide_populations_dev", (None, 0, None)),
                         ("dc_hip_reference_wide_nearest_dev", (None, None, None, None, None))):
            assert getattr(capi.lib, fn)(h._h, *args, None) == capi.DC_ERR_INVALID_ARGUMENT, "a sweep before any stage"
            assert fn in capi.lib.dc_hip_last_error().decode()
        with pytest.raises(capi.DensityLibraryError) as e:
            h.stage(Q)
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT and "dc_hip_reference_wide_stage_dev" in e.value.detail
        h.stage(Q[:200])
        with pytest.raises(capi.DensityLibraryError) as e:
            h.nearest(torch.zeros(200, device="cuda"))
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT and "dc_hip_reference_wide_nearest_dev" in e.value.detail
        h.stage(Q[:0])
        assert h.populations([1.0]).shape == (1, 0) and h.nearest()[0].shape == (0,) and h.info()[:4] == (0, 0, 0, 0)


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
import crosswideref as cw
import referencewideref as ref
assert capi.lib.dc_hip_canon_order().decode() == sys.argv[2]
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
Qb, Rb, r, _ = cw.boundary_sets(300, 1500, 100)
Ro = ref.reference_rows(1500, 100)
for what, Q, R, radii in (("boundary", Qb, Rb, [r]), ("ordinary", ref.ordinary_batch(Ro, 300), Ro, cw.radii_for(100, 3))):
    fe_q, fe_r = cw.fe_pair(len(Q), len(R))
    q, Rt, fq, fr = gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r)
    with dens.Reference(Rt, 300) as h:
        h.set_free_energies(fr)
        h.stage(q)
        assert torch.equal(h.populations(radii), dens.calculate_populations_against_wide(q, Rt, radii)), what
        assert h.info()[3] == 0 and h.info()[0] > 0
        assert all(same(a, b) for a, b in zip(h.nearest(fq), dens.nearest_reference_wide(q, Rt, fq, fr))), what
        assert h.info()[3] == 0 and h.info()[0] > 0
print("ok:", sys.argv[2])
"""


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_the_other_summation_orders(order):
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    env = dict(os.environ, DC_CANON_ORDER=order)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, order], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ok:" in r.stdout
