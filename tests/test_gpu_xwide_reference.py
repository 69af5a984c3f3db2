"""The resident reference for rows of 257..1024 columns (density.XWideReference, dc_hip_reference_xwide_*)
on the device: every output bit for bit against the unpruned cross sweeps of these widths
(calculate_populations_against_xwide, nearest_reference_xwide), and against variant="direct" where the direct kernels
answer -- batches in sequence on one handle, whatever came before, in every call order, through the gate of sixteen
columns per lane, at the edges, inside the pruning bounds formed from the device's own two orders, and with the exact-pair
counter inside the float64 range of the resident window.
Cases and premises: tests/xreferenceref.py, tests/test_reference_xwide_cases.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crossref
import crosswidepruneref as pr
import crosswideref as cw
import xcrosswidepruneref as xc
import xreferenceref as ref

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


def check_batch(dens, h, Q, Rt, radii=None, fe_q=None, fe_r=None, what="", order=("pops", "nn"), direct=False):
    """stage Q, run the sweeps named in `order`, each against the unpruned call (direct: and against the direct kernels);
    -> the info tuples of the sweeps"""
    q = gpu(Q)
    h.stage(q)
    infos = []
    for step in order:
        if step == "pops":
            got = h.populations(radii)
            assert torch.equal(got, dens.calculate_populations_against_xwide(q, Rt, radii)), (what, "populations", len(radii))
            if direct:
                assert torch.equal(got, dens.calculate_populations_against(q, Rt, radii, variant="direct")), (what, "populations, direct")
        else:
            fq, fr = (None, None) if fe_q is None else (gpu(fe_q), gpu(fe_r))
            got = h.nearest(fq)
            wants = [dens.nearest_reference_xwide(q, Rt, fq, fr)]
            if direct:
                wants.append(dens.nearest_reference(q, Rt, fq, fr, variant="direct"))
            for want in wants:
                for name, a, b in zip(("nn_idx", "nn_d2", "hd_idx", "hd_d2"), got, want):
                    assert same(a, b), (what, name, fe_q is not None, direct)
        infos.append(h.info())
    return infos


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_batches_in_sequence_on_one_handle(dens, n_cols):
    n_r = 1500
    R, Rt = reference(n_r, n_cols)
    radii9 = ref.radii9(n_cols)
    with dens.XWideReference(Rt, ref.MAX_BATCH) as h:
        perm_r0 = h.order()[1].clone()
        assert sorted(perm_r0.tolist()) == list(range(n_r))
        for k, n_q in enumerate(ref.BATCHES):
            Q = ref.ordinary_batch(R, n_q, seed=40 + k)
            fe_q, fe_r = cw.fe_pair(n_q, n_r, seed=17 + k)
            h.set_free_energies(gpu(fe_r))
            infos = []
            for n_rad, with_fe in ((1, True), (3, False), (9, True)):   # (nine radii: two launches)
                infos += check_batch(dens, h, Q, Rt, radii9[:n_rad], fe_q if with_fe else None, fe_r if with_fe else None,
                                     what=(n_cols, n_q, n_rad))
            for tiles, mfmas, _, answered, preparations in infos:
                assert answered == 0 and tiles > 0 and mfmas == cw.nm_for(n_cols) * tiles and preparations == 1, (n_q, infos)
            perm_q, perm_r = h.order()
            assert sorted(perm_q.tolist()) == list(range(n_q))
            assert torch.equal(perm_r, perm_r0), "the reference's order does not move"
        assert h.info()[4] == 1, "the reference was prepared once"


def test_a_reference_of_more_than_one_share(dens):
    R, Rt = reference(8320, 257)
    Q = ref.ordinary_batch(R, 1100, seed=44)
    fe_q, fe_r = cw.fe_pair(1100, 8320)
    with dens.XWideReference(Rt, 1100) as h:
        h.set_free_energies(gpu(fe_r))
        for tiles, mfmas, _, answered, _ in check_batch(dens, h, Q, Rt, cw.radii_for(257, 3), fe_q, fe_r, "8320 x 257"):
            assert answered == 0 and tiles > 0 and mfmas == cw.nm_for(257) * tiles


def test_history_does_not_matter(dens):
    R, Rt = reference(1500, 512)
    A, B = ref.headroom_batch(R, 300, seed=51), ref.ordinary_batch(R, 129, seed=52)
    radii = cw.radii_for(512, 3)
    fe_q, fe_r = cw.fe_pair(129, 1500)

    def run_b(h):
        h.stage(gpu(B))
        pops = h.populations(radii)
        ip = h.info()
        nn = h.nearest(gpu(fe_q))
        return pops, nn, ip, h.info()

    with dens.XWideReference(Rt, 300) as h1, dens.XWideReference(Rt, 300) as h2:
        for h in (h1, h2):
            h.set_free_energies(gpu(fe_r))
        check_batch(dens, h1, A, Rt, radii, what="A")
        after_a, fresh = run_b(h1), run_b(h2)
    assert torch.equal(after_a[0], fresh[0]) and all(same(a, b) for a, b in zip(after_a[1], fresh[1]))
    assert after_a[2][:2] == fresh[2][:2] and after_a[3][:2] == fresh[3][:2], "tiles and mfmas"


def test_call_orders_on_one_staged_batch(dens):
    R, Rt = reference(1500, 257)
    Q = ref.ordinary_batch(R, 300, seed=61)
    fe_q, fe_r = cw.fe_pair(300, 1500, seed=3)
    r3 = cw.radii_for(257, 3)
    with dens.XWideReference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        check_batch(dens, h, Q, Rt, r3, fe_q, fe_r, "populations twice", ("pops", "pops"))
        check_batch(dens, h, Q, Rt, r3, fe_q, fe_r, "nn -> pops", ("nn", "pops"))
        check_batch(dens, h, Q, Rt, r3, fe_q, fe_r, "pops -> nn", ("pops", "nn"))
        assert h.info()[4] == 1


FLAWS = [("nan", 300), ("inf", 300), ("beyond", 300), ("tail", 300), ("nan", 512), ("inf", 512), ("beyond", 512), ("tail", 512),
         ("tail", 257), ("tail", 1023)]


@pytest.mark.parametrize("flaw,n_cols", FLAWS)
def test_a_flagged_batch_goes_to_the_direct_kernels_and_the_next_one_does_not(dens, flaw, n_cols):
    """300 columns: the generic direct kernel answers; 512 and 1023: the column-chunked one (beyond 400 columns).  The tail
    outlier is beyond M_res in ONE column >= 256: a gate reading four columns per lane would let it through to the matrix
    cores under a scale that does not cover it."""
    R, Rt = reference(1500, n_cols)
    radii = cw.radii_for(n_cols, 3)
    fe_q, fe_r = cw.fe_pair(300, 1500)
    if flaw == "beyond":
        Q = ref.beyond_batch(R, 300)
    elif flaw == "tail":
        Q = ref.tail_outlier_batch(R, 300)[0]
    else:
        Q = ref.ordinary_batch(R, 300)
        Q[153, n_cols - 1] = np.nan if flaw == "nan" else np.inf
    with dens.XWideReference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        for info in check_batch(dens, h, Q, Rt, radii, fe_q, fe_r, flaw, direct=True):
            assert info[:4] == (0, 0, 0, 2), info
        for info in check_batch(dens, h, ref.ordinary_batch(R, 300, seed=5), Rt, radii, fe_q, fe_r, "after " + flaw):
            assert info[3] == 0 and info[0] > 0, info


@pytest.mark.parametrize("n_cols", [300, 1024])
def test_a_batch_inside_the_headroom_and_outside_the_extent_runs_on_the_matrix_cores(dens, n_cols):
    R, Rt = reference(1500, n_cols)
    Q = ref.headroom_batch(R, 300)
    fe_q, fe_r = cw.fe_pair(300, 1500)
    with dens.XWideReference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        for info in check_batch(dens, h, Q, Rt, cw.radii_for(n_cols, 3), fe_q, fe_r, "headroom"):
            assert info[3] == 0 and info[0] > 0, info


@pytest.mark.parametrize("flaw,n_cols", [("nan reference", 300), ("big reference", 512)])
def test_a_flagged_reference_opens_and_every_batch_is_answered_by_the_direct_kernels(dens, flaw, n_cols):
    R = reference(1500, n_cols)[0]
    _, Rf = cw.flawed_sets(R[:8], R, flaw)
    Rt = gpu(Rf)
    fe_q, fe_r = cw.fe_pair(129, 1500)
    with dens.XWideReference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        for k in range(2):
            for info in check_batch(dens, h, ref.ordinary_batch(R, 129, seed=70 + k), Rt, cw.radii_for(n_cols, 3), fe_q, fe_r, flaw,
                                    direct=True):
                assert info[:4] == (0, 0, 0, 1), info


@pytest.mark.parametrize("side", ["fe_ref", "fe_query"])
def test_a_nan_free_energy_sends_the_neighbour_sweep_alone_to_the_direct_kernel(dens, side):
    R, Rt = reference(1500, 512)
    Q = ref.ordinary_batch(R, 300)
    fe_q, fe_r = cw.fe_pair(300, 1500)
    (fe_r if side == "fe_ref" else fe_q)[77] = np.nan
    with dens.XWideReference(Rt, 300) as h:
        h.set_free_energies(gpu(fe_r))
        for order in (("pops", "nn"), ("nn", "pops")):
            infos = dict(zip(order, check_batch(dens, h, Q, Rt, cw.radii_for(512, 3), fe_q, fe_r, side, order, direct=True)))
            assert infos["nn"][:4] == (0, 0, 0, 3), infos
            assert infos["pops"][3] == 0 and infos["pops"][0] > 0, infos
        clean_q, clean_r = cw.fe_pair(300, 1500)
        h.set_free_energies(gpu(clean_r))
        assert check_batch(dens, h, Q, Rt, None, clean_q, clean_r, "clean again", ("nn",))[0][3] == 0


def test_edges_through_the_resident_path(dens):
    cases = []
    Q, R, r, _ = cw.boundary_sets(300, 1500, 512)
    cases.append(("boundary", Q, R, [r]))
    Q, R, *_ = cw.ties_sets(300, 1500, 257)
    cases.append(("ties", Q, R, cw.radii_for(257, 3)))
    Q, R, r, _ = xc.margin_sets(300)
    cases.append(("margin", Q, R, [r]))
    R1500 = reference(1500, 1024)[0]
    cases.append(("reference of 1 row", R1500[5:305], R1500[:1], cw.radii_for(1024, 3)))
    # (rows of the same cloud: all within 1.1 M_ref of the 129 rows' mean, so the matrix cores answer)
    cases.append(("reference of 129 rows", R1500[200:500], R1500[:129], cw.radii_for(1024, 3)))
    cases.append(("the batch is the reference", R1500, R1500, cw.radii_for(1024, 3)))
    for what, Q, R, radii in cases:
        fe_q, fe_r = cw.fe_pair(len(Q), len(R))
        Rt = gpu(R)
        d2 = crossref.block_d2(the_probe(), Q, R)
        with dens.XWideReference(Rt, len(Q)) as h:
            h.set_free_energies(gpu(fe_r))
            check_batch(dens, h, Q, Rt, radii, fe_q, fe_r, what)
            assert (crossref.host(h.populations(radii)) == crossref.expect_pops(d2, radii)).all(), (what, "probe, populations")
            crossref.same_nn(h.nearest(gpu(fe_q)), crossref.expect_nn(d2, fe_q, fe_r), what + ", probe")
            check_batch(dens, h, Q, Rt, radii, None, None, what + ", nn only", ("nn",))


@pytest.mark.parametrize("n_cols", ref.COLS)
def test_the_sweeps_prune_and_the_exact_path_takes_the_pairs_of_the_resident_window(dens, n_cols):
    """`tiles` between the bounds formed from the device's two orders with the constants of these widths, strictly below
    the unpruned count; `exact_pairs` between the float64 counts of the pairs within (1 - f) and (1 + f) of the window's
    half-width -- the half-width restated in numpy from guard_band with M_res = 4 M_ref, f twice the worst |error| / band
    measured at the width (xreferenceref.F_EXACT).  A window formed from M_ref, or one twice too wide, falls outside the
    range (tests/test_reference_xwide_cases.py)."""
    Q, R, fe_q, fe_r = ref.split_case(1500, 1500, n_cols)
    radii, f = ref.radii_for(n_cols), ref.F_EXACT[n_cols]
    Rt = gpu(R)
    with dens.XWideReference(Rt, len(Q)) as h:
        h.set_free_energies(gpu(fe_r))
        pops_info, nn_info = check_batch(dens, h, Q, Rt, radii, fe_q, fe_r, "pruning")
        perm_q, perm_r = (p.cpu().numpy().astype(np.int64) for p in h.order())
    g = pr.gaps(Q, R, perm_q, perm_r)
    lo, hi = pr.tile_bounds(Q, R, perm_q, perm_r, radii)
    print(f"D={n_cols} populations: tiles {pops_info[0]} in [{lo}, {hi}] of {16 * g.size}")
    assert pops_info[3] == 0 and lo <= pops_info[0] <= hi < 16 * g.size
    lo, hi = xc.nn_tile_bounds(Q, R, fe_q, fe_r, perm_q, perm_r)
    print(f"D={n_cols} neighbours: tiles {nn_info[0]} in [{lo}, {hi}] of {16 * g.size}")
    assert nn_info[3] == 0 and lo <= nn_info[0] <= hi < 16 * g.size
    (lower, _), (inside, _), (_, upper) = ref.window_counts(n_cols, Q, R, perm_q, perm_r, radii, [1.0 - f, 1.0, 1.0 + f])
    exact = pops_info[2]
    print(f"D={n_cols}: {exact} exact pairs of {1024 * pops_info[0]} evaluated = {100.0 * exact / (1024 * pops_info[0]):.3f} %; "
          f"float64 count in the window {inside}, at (1 -/+ {f:.4f}) of it {lower} / {upper}")
    assert lower <= exact <= upper, (lower, exact, upper)


def test_reference_assign_equals_assign_frames_xwide_pruned(dens):
    R, Rt = reference(1500, 300)
    Q = np.concatenate([ref.ordinary_batch(R, 2000, seed=81), ref.headroom_batch(R, 500, seed=82)])
    states = (np.arange(1500) % 7).astype(np.int32)
    radius = cw.radii_for(300, 1)[0]
    want = dens.assign_frames_xwide_pruned(gpu(Q), Rt, radius, states, pruned_neighbours=True)
    with dens.XWideReference(Rt, 1000, radius=radius, ref_states=states) as h:
        got = h.assign(gpu(Q))   # three chunks: 1000, 1000, 500
        on_device = h.assign_device(gpu(Q))
        assert h.info()[4] == 1
    for g in (got, on_device):
        assert set(g) == set(want)
        for key in want:
            if key == "max_pop":
                assert g[key] == want[key]
            else:
                assert same(g[key], want[key]), key
    assert int(want["pops"].max()) > 0 and len(torch.unique(want["states"])) > 1, "the case says something"
    for n_cols in (256, 1025):
        with pytest.raises(ValueError, match="257..1024"):
            dens.XWideReference(torch.zeros((10, n_cols), device="cuda"), 10)


def test_refusals_of_a_handle(dens):
    from clustering_amd import capi
    R, Rt = reference(1500, 300)
    Q = gpu(ref.ordinary_batch(R, 300))
    with dens.XWideReference(Rt, 200) as h:
        for call in (lambda: h.populations([1.0]), lambda: h.nearest()):
            with pytest.raises(ValueError):
                call()
        for fn, args in (("dc_hip_reference_xwide_populations_dev", (None, 0, None)),
                         ("dc_hip_reference_xwide_nearest_dev", (None, None, None, None, None))):
            assert getattr(capi.lib, fn)(h._h, *args, None) == capi.DC_ERR_INVALID_ARGUMENT, "a sweep before any stage"
            assert fn in capi.lib.dc_hip_last_error().decode()
        with pytest.raises(capi.DensityLibraryError) as e:
            h.stage(Q)
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT and "dc_hip_reference_xwide_stage_dev" in e.value.detail
        h.stage(Q[:200])
        with pytest.raises(capi.DensityLibraryError) as e:
            h.nearest(torch.zeros(200, device="cuda"))
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT and "dc_hip_reference_xwide_nearest_dev" in e.value.detail
        # a refused call leaves the handle usable
        radii = cw.radii_for(300, 3)
        assert torch.equal(h.populations(radii), dens.calculate_populations_against_xwide(Q[:200].contiguous(), Rt, radii))
        assert h.info()[3] == 0 and h.info()[0] > 0
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
import xreferenceref as ref
assert capi.lib.dc_hip_canon_order().decode() == sys.argv[2]
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
Q, R, r, _ = cw.boundary_sets(300, 1500, 512)
fe_q, fe_r = cw.fe_pair(len(Q), len(R))
q, Rt, fq, fr = gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r)
with dens.XWideReference(Rt, 300) as h:
    h.set_free_energies(fr)
    h.stage(q)
    assert torch.equal(h.populations([r]), dens.calculate_populations_against_xwide(q, Rt, [r]))
    assert h.info()[3] == 0 and h.info()[0] > 0
    assert all(same(a, b) for a, b in zip(h.nearest(fq), dens.nearest_reference_xwide(q, Rt, fq, fr)))
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
