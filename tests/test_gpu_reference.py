"""The resident reference of the pruned cross sweeps for rows of 1..64 columns (density.NarrowReference,
dc_hip_reference_*) on the device: every output bit for bit against the exact kernels
(calculate_populations_against(variant="direct"), nearest_reference(variant="direct")) -- batches in sequence on one
handle, whatever came before, in every call order, through the gate, at boundaries and ties, inside the pruning bounds
formed from the device's own orders.  No case but the gate's may pass on the direct kernels: each asserts that the matrix
cores answered (answered == 0) and evaluated something (tiles > 0).
Cases and premises: tests/referenceref.py, tests/test_reference_cases.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crossbigref as big
import referenceref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def dens():
    from clustering_amd import density
    return density


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same(a, b):
    """bit for bit: integers as they are, floats by their bits; None only equals None"""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def reference(D, n=ref.N_REF):
    R = ref.reference_rows(D, n)
    return R, gpu(R)


def open_(dens, Rt, max_batch, D, **kw):
    kw.setdefault("max_radius", ref.max_radius(D))
    return dens.NarrowReference(Rt, max_batch, **kw)


def check_batch(dens, h, Q, Rt, radii=None, fe_q=None, fe_r=None, what="", order=("pops", "nn")):
    """stage Q, run the sweeps named in `order`, each against the exact kernels; -> the info tuples of the sweeps"""
    q = gpu(Q)
    h.stage(q)
    infos = []
    for step in order:
        if step == "pops":
            got = h.populations(radii)
            want = dens.calculate_populations_against(q, Rt, radii, variant="direct")
            assert torch.equal(got, want), (what, "populations", len(radii))
        else:
            fq, fr = (None, None) if fe_q is None else (gpu(fe_q), gpu(fe_r))
            got = h.nearest(fq)
            want = dens.nearest_reference(q, Rt, fq, fr, variant="direct")
            for name, a, b in zip(("nn_idx", "nn_d2", "hd_idx", "hd_d2"), got, want):
                assert same(a, b), (what, name, fe_q is not None)
        infos.append(h.info())
    return infos


def on_the_matrix_cores(infos, what=""):
    for tiles, mfmas, _, answered, preparations in infos:
        assert answered == 0 and tiles > 0 and mfmas > 0 and preparations == 1, (what, infos)


@pytest.mark.parametrize("D", ref.WIDTHS)
def test_batches_in_sequence_on_one_handle(dens, D):
    R, Rt = reference(D)
    radii9 = ref.radii(D, 9)   # (the largest of them is max_radius itself)
    with open_(dens, Rt, ref.MAX_BATCH, D) as h:
        perm_r0 = None
        for k, n_q in enumerate(ref.BATCHES):
            Q = ref.ordinary_batch(R, n_q, seed=40 + k)
            fe_q, fe_r = ref.fe_pair(n_q, len(R), seed=17 + k)
            # every size with 1, 3 and 9 radii, with free energies (new ones per batch) and without
            h.set_free_energies(gpu(fe_r))
            infos = []
            for n_rad, with_fe in ((1, True), (3, False), (9, True)):
                infos += check_batch(dens, h, Q, Rt, radii9[:n_rad], fe_q if with_fe else None, fe_r if with_fe else None,
                                     what=(D, n_q, n_rad))
            on_the_matrix_cores(infos, (D, n_q))
            for which in (0, 1):
                perm_q, perm_r = h.order(which)
                assert sorted(perm_q.tolist()) == list(range(n_q)) and sorted(perm_r.tolist()) == list(range(len(R)))
            perm_r = h.order(0)[1]
            perm_r0 = perm_r if perm_r0 is None else perm_r0
            assert torch.equal(perm_r, perm_r0), "the population order of the reference does not move"
        assert h.info()[4] == 1, "the reference was prepared once"


def test_history_does_not_matter(dens):
    R, Rt = reference(10)
    A, B = ref.headroom_batch(R, 300, seed=51), ref.ordinary_batch(R, 193, seed=52)
    radii = ref.radii(10, 3)
    fe_q, fe_r = ref.fe_pair(193, len(R))

    def run_b(h):
        h.stage(gpu(B))
        pops = h.populations(radii)
        ip = h.info()
        nn = h.nearest(gpu(fe_q))
        return pops, nn, ip, h.info()

    with open_(dens, Rt, 300, 10) as h1, open_(dens, Rt, 300, 10) as h2:
        for h in (h1, h2):
            h.set_free_energies(gpu(fe_r))
        on_the_matrix_cores(check_batch(dens, h1, A, Rt, radii, what="A"))
        after_a, fresh = run_b(h1), run_b(h2)
        h1.stage(gpu(A))
        again = run_b(h1)
    for other in (fresh, again):
        assert torch.equal(after_a[0], other[0]) and all(same(a, b) for a, b in zip(after_a[1], other[1]))
        assert after_a[2][:2] == other[2][:2] and after_a[3][:2] == other[3][:2], "tiles and mfmas"
    on_the_matrix_cores(after_a[2:])


def test_call_orders_on_one_staged_batch(dens):
    R, Rt = reference(10)
    Q = ref.ordinary_batch(R, 300, seed=61)
    fe_q, fe_r = ref.fe_pair(300, len(R), seed=3)
    fe_r2 = ref.fe_pair(300, len(R), seed=4)[1]
    r3, r9 = ref.radii(10, 3), ref.radii(10, 9)

    def direct_pops(q, radii):
        return dens.calculate_populations_against(q, Rt, radii, variant="direct")

    def direct_nn(q, fq=None, fr=None):
        return dens.nearest_reference(q, Rt, fq, fr, variant="direct")

    with open_(dens, Rt, 300, 10) as h:
        h.set_free_energies(gpu(fe_r))
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, r3, fe_q, fe_r, "pops -> nn", ("pops", "nn")))
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, r3, fe_q, fe_r, "nn -> pops", ("nn", "pops")))
        q = gpu(Q)
        h.stage(q)
        for radii in (r3, r9[3:], r9, r3[:1]):
            assert torch.equal(h.populations(radii), direct_pops(q, radii)), "populations twice"
            on_the_matrix_cores([h.info()])
        want = direct_nn(q, gpu(fe_q), gpu(fe_r))
        for _ in range(2):
            assert all(same(a, b) for a, b in zip(h.nearest(gpu(fe_q)), want)), "nearest twice"
            on_the_matrix_cores([h.info()])
        assert all(same(a, b) for a, b in zip(h.nearest(), direct_nn(q))), "nn only, after the full call"
        assert torch.equal(h.populations(r3), direct_pops(q, r3)), "populations after the neighbours"
        # new free energies of the reference between two nearest calls on the SAME staged batch
        h.set_free_energies(gpu(fe_r2))
        assert all(same(a, b) for a, b in zip(h.nearest(gpu(fe_q)), direct_nn(q, gpu(fe_q), gpu(fe_r2)))), "new free energies"
        on_the_matrix_cores([h.info()])
        assert torch.equal(h.populations(r3), direct_pops(q, r3)), "populations after new free energies"
        assert h.info()[4] == 1


@pytest.mark.parametrize("D", [3, 10])
def test_small_references_and_the_reference_as_its_own_batch(dens, D):
    full = reference(D)[0]
    radii = ref.radii(D, 3)
    # a reference of one row: M_ref = 0, so only copies of that row pass the gate -- they do, on the matrix cores
    one, copies = full[:1], np.repeat(full[:1], 5, axis=0)
    with open_(dens, gpu(one), 8, D) as h:
        on_the_matrix_cores(check_batch(dens, h, copies, gpu(one), radii, what="reference of 1 row"))
        assert (h.populations(radii) == 1).all() and (h.nearest()[0] == 0).all() and (h.nearest()[1] == 0).all()
    # 33 rows: one tile and one row of the next
    R33 = full[:33]
    fe_q, fe_r = ref.fe_pair(33, 33)
    with open_(dens, gpu(R33), 64, D) as h:
        h.set_free_energies(gpu(fe_r))
        on_the_matrix_cores(check_batch(dens, h, R33[::-1].copy(), gpu(R33), radii, fe_q, fe_r, "reference of 33 rows"))
    # the reference as its own batch, with a few duplicated rows: the self pair is counted, the nearest frame of a row is its
    # lowest-index copy at d2 = 0
    R = full.copy()
    R[100:104] = R[3:7]
    Rt = gpu(R)
    with open_(dens, Rt, len(R), D) as h:
        on_the_matrix_cores(check_batch(dens, h, R, Rt, radii, what="the batch is the reference"))
        pops, (nn_idx, nn_d2, _, _) = h.populations(radii), h.nearest()
        assert (pops >= 1).all() and (pops[:, 100:104] >= 2).all()
        want = np.arange(len(R))
        want[100:104] = np.arange(3, 7)
        assert (nn_idx.cpu().numpy() == want).all() and (nn_d2 == 0).all()


def test_a_reference_large_enough_for_several_shares(dens):
    """57 600 rows = 1 800 reference tiles: the neighbour sweep's share floor (kNnShareFloor = 900 tiles) admits two shares
    from there on; 8 320 rows (260 tiles) still run in one.  The population sweep splits it in seven (256 tiles per share):
    its counts are then added with atomics into the zero-filled array."""
    D, n_r, n_q = 3, 57600, 300
    assert big.nn_shares(n_q, 8320, D) == 1 and big.nn_shares(n_q, n_r - 32, D) == 1 and big.nn_shares(n_q, n_r, D) == 2
    assert big.pop_shares(n_q, n_r, D) == 7
    R, Rt = reference(D, n_r)
    Q = ref.ordinary_batch(R, n_q, seed=71)
    fe_q, fe_r = ref.fe_pair(n_q, n_r)
    with open_(dens, Rt, n_q, D) as h:
        h.set_free_energies(gpu(fe_r))
        pops_info, nn_info = check_batch(dens, h, Q, Rt, ref.radii(D, 3), fe_q, fe_r, "several shares")
        nn_only = check_batch(dens, h, Q, Rt, None, None, None, "several shares, nn only", ("nn",))[0]
    on_the_matrix_cores([pops_info, nn_info, nn_only])
    assert nn_info[2] == 2 and nn_only[2] == 2 and pops_info[2] == 0, "shares of the last sweep"


@pytest.mark.parametrize("flaw", ["nan", "inf", "beyond"])
def test_a_flagged_batch_goes_to_the_direct_kernels_and_the_next_one_does_not(dens, flaw):
    R, Rt = reference(10)
    radii = ref.radii(10, 3)
    fe_q, fe_r = ref.fe_pair(300, len(R))
    if flaw == "beyond":
        Q = ref.beyond_batch(R, 300)
    else:
        Q = ref.ordinary_batch(R, 300)
        Q[153, 9] = np.nan if flaw == "nan" else np.inf
    with open_(dens, Rt, 300, 10) as h:
        h.set_free_energies(gpu(fe_r))
        for info in check_batch(dens, h, Q, Rt, radii, fe_q, fe_r, flaw):
            assert info[:4] == (0, 0, 0, 2), info
        on_the_matrix_cores(check_batch(dens, h, ref.ordinary_batch(R, 300, seed=5), Rt, radii, fe_q, fe_r, "after " + flaw))


@pytest.mark.parametrize("D", [1, 7, 10, 64])
def test_a_batch_inside_the_headroom_and_outside_the_extent_runs_on_the_matrix_cores(dens, D):
    R, Rt = reference(D)
    Q = ref.headroom_batch(R, 300)
    fe_q, fe_r = ref.fe_pair(300, len(R))
    with open_(dens, Rt, 300, D) as h:
        h.set_free_energies(gpu(fe_r))
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, ref.radii(D, 3), fe_q, fe_r, "headroom"))


@pytest.mark.parametrize("flaw", ["nan", "inf", "big"])
def test_a_flagged_reference_opens_and_every_batch_is_answered_by_the_direct_kernels(dens, flaw):
    R = reference(10)[0]
    Rf = ref.flawed_reference(R, flaw)
    Rt = gpu(Rf)
    fe_q, fe_r = ref.fe_pair(193, len(R))
    with open_(dens, Rt, 300, 10) as h:
        h.set_free_energies(gpu(fe_r))
        for k in range(2):
            for info in check_batch(dens, h, ref.ordinary_batch(R, 193, seed=70 + k), Rt, ref.radii(10, 3), fe_q, fe_r, flaw):
                assert info[:4] == (0, 0, 0, 1), info


@pytest.mark.parametrize("side", ["fe_ref", "fe_query"])
def test_a_nan_free_energy_sends_the_neighbour_sweep_alone_to_the_direct_kernel(dens, side):
    R, Rt = reference(10)
    Q = ref.ordinary_batch(R, 300)
    fe_q, fe_r = ref.fe_pair(300, len(R))
    (fe_r if side == "fe_ref" else fe_q)[77] = np.nan
    with open_(dens, Rt, 300, 10) as h:
        h.set_free_energies(gpu(fe_r))
        for order in (("pops", "nn"), ("nn", "pops")):
            infos = dict(zip(order, check_batch(dens, h, Q, Rt, ref.radii(10, 3), fe_q, fe_r, side, order)))
            assert infos["nn"][:4] == (0, 0, 0, 3), infos
            on_the_matrix_cores([infos["pops"]])
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, None, None, None, "neighbours without free energies read none", ("nn",)))
        clean_q, clean_r = ref.fe_pair(300, len(R))
        h.set_free_energies(gpu(clean_r))
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, None, clean_q, clean_r, "clean again", ("nn",)))


@pytest.mark.parametrize("D", [3, 10])
def test_boundaries_and_ties(dens, D):
    # pairs exactly at r^2 (strict <), and one float either side of it
    Q, R, trio = ref.boundary_case(D)
    fe_q, fe_r = ref.fe_pair(len(Q), len(R))
    Rt = gpu(R)
    with open_(dens, Rt, len(Q), D, max_radius=max(trio)) as h:
        h.set_free_energies(gpu(fe_r))
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, trio, fe_q, fe_r, "boundary"))
        pops = h.populations(trio).cpu().numpy().astype(np.int64)
        d2 = ref.d2_exact(Q, R)
        level = float(F32(trio[0]) * F32(trio[0]))
        assert (pops[0] == (d2 < level).sum(axis=1)).all() and (pops[2] == pops[0]).all(), "at the level: not inside"
        assert (pops[1] == (d2 <= level).sum(axis=1)).all() and (pops[1] > pops[0]).any(), "one float above: inside"
    # duplicates of reference rows, queries tied between two references, fe_query equal to fe_ref
    Q, R, fe_q, fe_r = ref.tie_case(D)
    Rt = gpu(R)
    with open_(dens, Rt, len(Q), D, max_radius=1.0) as h:
        h.set_free_energies(gpu(fe_r))
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, [0.0625, 0.125, 1.0], fe_q, fe_r, "ties"))
        on_the_matrix_cores(check_batch(dens, h, Q, Rt, None, None, None, "ties, nn only", ("nn",)))
        nn_idx, nn_d2, hd_idx, _ = (t.cpu().numpy() for t in h.nearest(gpu(fe_q)))
        d2 = ref.d2_exact(Q, R)
        assert (nn_idx == np.argmax(d2 == d2.min(axis=1)[:, None], axis=1)).all(), "the lowest row of a tie wins"
        assert (nn_idx[96:128] < 32).all() and (nn_d2[96:] == 0).all(), "of a row and its copy, the row"
        lower = fe_r[None, :] < fe_q[:, None]
        masked = np.where(lower, d2, np.inf)
        assert (hd_idx == np.argmax(masked == masked.min(axis=1)[:, None], axis=1)).all(), "equal free energy is not lower"


def test_radii_against_max_radius(dens):
    from clustering_amd import capi
    R, Rt = reference(10)
    q = gpu(ref.ordinary_batch(R, 300))
    r = ref.radius(10)
    with open_(dens, Rt, 300, 10, max_radius=r) as h:
        h.stage(q)
        assert torch.equal(h.populations([r, 0.5 * r]), dens.calculate_populations_against(q, Rt, [r, 0.5 * r], variant="direct"))
        on_the_matrix_cores([h.info()])
        with pytest.raises(capi.DensityLibraryError) as e:
            h.populations([0.5 * r, float(np.nextafter(F32(r), F32(np.inf))) * 1.001])
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT and "dc_hip_reference_populations_dev" in e.value.detail
    with open_(dens, Rt, 300, 10, max_radius=float("inf")) as h:
        h.stage(q)
        assert torch.equal(h.populations([r]), dens.calculate_populations_against(q, Rt, [r], variant="direct"))
        assert h.info()[3] == 0 and h.info()[0] > 0
        assert (h.populations([float("inf")]) == len(R)).all()


def test_the_sweeps_prune_and_the_restated_orders_are_the_devices(dens):
    D = 10
    R, Rt = reference(D)
    Q = ref.ordinary_batch(R, 1100, seed=91)
    fe_q, fe_r = ref.fe_pair(len(Q), len(R))
    r = ref.radius(D)
    tq = big.tq_of(big.nm_for(D))
    T_q, T_r = big.tiles(len(Q)), big.tiles(len(R))
    with open_(dens, Rt, len(Q), D) as h:
        (pops_info,) = check_batch(dens, h, Q, Rt, [r], what="pruning", order=("pops",))
        dev = [[p.cpu().numpy().astype(np.int64) for p in h.order(which)] for which in (0, 1)]
        for which in (0, 1):
            for got, want in zip(dev[which], ref.orders(Q, R, which)):
                assert (got == want).all(), ("the restated order", which)
        (nn_only,) = check_batch(dens, h, Q, Rt, what="pruning, nn only", order=("nn",))
        h.set_free_energies(gpu(fe_r))
        (nn_info,) = check_batch(dens, h, Q, Rt, None, fe_q, fe_r, "pruning, neighbours", ("nn",))
        perm_q1, perm_r1 = (p.cpu().numpy().astype(np.int64) for p in h.order(1))
        for got, want in zip((perm_q1, perm_r1), ref.orders(Q, R, 1, fe_r)):
            assert (got == want).all(), "the restated (cell, free energy) order"
        assert (h.order(0)[1].cpu().numpy() == dev[0][1]).all(), "the population side is not prepared again"
    on_the_matrix_cores([pops_info, nn_only, nn_info])
    need = ref.pairs_within(Q, R, dev[0][0], dev[0][1], r, tq)
    print(f"populations: tiles {pops_info[0]} of {T_q * T_r}, at least {tq} x {need}; neighbours: {nn_only[0]}, {nn_info[0]}")
    assert tq * need <= pops_info[0] < T_q * T_r, "every (group, tile) pair within the radius is evaluated; the blobs apart are not"
    assert nn_only[0] < T_q * T_r and nn_info[0] < T_q * T_r


def test_assign_equals_assign_frames(dens):
    D = 10
    R, Rt = reference(D)
    Q = np.concatenate([ref.ordinary_batch(R, 2000, seed=81), ref.headroom_batch(R, 500, seed=82)])
    states = (np.arange(len(R)) % 7).astype(np.int32)
    radius = ref.radius(D)
    want = dens.assign_frames(gpu(Q), Rt, radius, states, variant="cross_pruned", pruned_neighbours=True)
    with dens.NarrowReference(Rt, 1000, radius=radius, ref_states=states) as h:
        assert h.max_radius == radius
        got = h.assign(gpu(Q))   # three chunks: 1000, 1000, 500
        assert h.info()[3] == 0 and h.info()[0] > 0 and h.info()[4] == 1
    assert set(got) == set(want)
    for key in want:
        if key == "max_pop":
            assert got[key] == want[key]
        else:
            assert same(got[key], want[key]), key
    # what the constructor can refuse it refuses before it opens a handle
    for kwargs in ({"radius": radius}, {"ref_states": states}, {"radius": radius, "ref_states": states[:-1]}, {}):
        with pytest.raises(ValueError):
            dens.NarrowReference(Rt, 1000, **kwargs)
    with pytest.raises(ValueError):
        dens.NarrowReference(Rt, 0, max_radius=1.0)
    with pytest.raises(ValueError):
        dens.Reference(Rt, 1000)   # (the wide handle keeps refusing these widths)


def test_refusals_of_a_handle(dens):
    from clustering_amd import capi
    R, Rt = reference(10)
    Q = gpu(ref.ordinary_batch(R, 300))
    with open_(dens, Rt, 200, 10) as h:
        for call in (lambda: h.populations([0.1]), lambda: h.nearest()):
            with pytest.raises(ValueError):
                call()
        for fn, args in (("dc_hip_reference_populations_dev", (None, 0, None)),
                         ("dc_hip_reference_nearest_dev", (None, None, None, None, None))):
            assert getattr(capi.lib, fn)(h._h, *args, None) == capi.DC_ERR_INVALID_ARGUMENT, "a sweep before any stage"
            assert fn in capi.lib.dc_hip_last_error().decode()
        with pytest.raises(capi.DensityLibraryError) as e:
            h.stage(Q)
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT and "dc_hip_reference_stage_dev" in e.value.detail
        h.stage(Q[:200])
        with pytest.raises(capi.DensityLibraryError) as e:
            h.nearest(torch.zeros(200, device="cuda"))
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT and "dc_hip_reference_nearest_dev" in e.value.detail
        with pytest.raises(capi.DensityLibraryError) as e:
            h.order(2)
        assert e.value.status == capi.DC_ERR_INVALID_ARGUMENT
        h.stage(Q[:0])
        assert h.populations([0.1]).shape == (1, 0) and h.nearest()[0].shape == (0,)
    with pytest.raises(ValueError, match="closed"):
        h.stage(Q[:200])
    with pytest.raises(ValueError, match="closed"):
        h.info()


CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from clustering_amd import capi, density as dens
import referenceref as ref
assert capi.lib.dc_hip_canon_order().decode() == sys.argv[2]
gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
Qb, Rb, trio = ref.boundary_case(10)
Ro = ref.reference_rows(10)
for what, Q, R, radii in (("boundary", Qb, Rb, trio), ("ordinary", ref.ordinary_batch(Ro, 300), Ro, ref.radii(10, 3))):
    fe_q, fe_r = ref.fe_pair(len(Q), len(R))
    q, Rt, fq, fr = gpu(Q), gpu(R), gpu(fe_q), gpu(fe_r)
    with dens.NarrowReference(Rt, len(Q), max_radius=max(radii)) as h:
        h.set_free_energies(fr)
        h.stage(q)
        assert torch.equal(h.populations(radii), dens.calculate_populations_against(q, Rt, radii, variant="direct")), what
        assert h.info()[3] == 0 and h.info()[0] > 0
        assert all(same(a, b) for a, b in zip(h.nearest(fq), dens.nearest_reference(q, Rt, fq, fr, variant="direct"))), what
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
