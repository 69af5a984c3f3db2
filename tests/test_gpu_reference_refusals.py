"""The refusals of the two resident reference handles that need an open handle (dc_hip_reference_*, 1..64 columns;
dc_hip_reference_wide_*, 65..256), and those of dc_hip_assign_open[_wide]_dev on one: status code and full
dc_hip_last_error() text, in one fixed sequence of calls per kind on one handle at the smallest shapes that open (a
reference of 40 x 3 and of 40 x 70, batches of at most 8).  Both kinds share one struct and one body per step; the
sequence pins what each body refuses, in which order, and in whose name.  Every case is an argument refusal: nothing here
reaches a sweep but the last step, which shows that the refused calls left the handle usable -- the staged batch of 8 rows
gives the populations and neighbours of the per-call pruned entry points bit for bit.

The expected values were RECORDED on the device from the library of the commit before the handles were folded, not derived
from the code under test:

    DC_LIB_PATH=<that commit's libdcdensity.so> python tests/test_gpu_reference_refusals.py

prints the EXPECTED literal at the end of this file.  (The refusals that need no handle: tests/test_capi_reference_refusals.py.)"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, WORKSPACE = 0, -1, -5
N_REF, MAX_BATCH = 40, 8
# kind -> (entry points' prefix, the assigner's open, columns, the radius of the sweeps = max_radius of the narrow handle)
KINDS = {"narrow": ("dc_hip_reference_", "dc_hip_assign_open_dev", 3, 1.0),
         "wide": ("dc_hip_reference_wide_", "dc_hip_assign_open_wide_dev", 70, 12.0)}


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def data(kind):
    """reference [40, D], nine query rows (a batch of 8, and one row too many), free energies of both sides, states"""
    D = KINDS[kind][2]
    rng = np.random.default_rng(7 + D)
    R = rng.standard_normal((N_REF, D)).astype(np.float32)
    Q = (R[rng.integers(0, N_REF, MAX_BATCH + 1)] + 0.3 * rng.standard_normal((MAX_BATCH + 1, D))).astype(np.float32)
    fe_r, fe_q = rng.random(N_REF).astype(np.float32), rng.random(MAX_BATCH).astype(np.float32)
    return R, Q, fe_r, fe_q, rng.integers(1, 5, N_REF).astype(np.int32)


def sequence(lib, kind):
    """-> ({step: [status, text]} in the order of the calls, (pops, nn_idx, nn_d2, hd_idx, hd_d2) of the last batch)"""
    api, assign_open, D, radius = KINDS[kind]
    narrow = kind == "narrow"
    R, Q, fe_r, fe_q, states = (gpu(a) for a in data(kind))
    f = lambda step: getattr(lib, api + step)   # noqa: E731
    got = {}

    def note(step, rc):
        assert step not in got
        got[step] = [rc, lib.dc_hip_last_error().decode() if rc else ""]

    def rad(r):
        return np.array([r], dtype=np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    need = f("workspace_bytes")(N_REF, D, MAX_BATCH)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    h = ctypes.c_void_p()
    rc = f("open_dev")(ptr(R), N_REF, D, MAX_BATCH, *((radius,) if narrow else ()), ptr(ws), need, None, ctypes.byref(h))
    assert rc == OK and h.value, lib.dc_hip_last_error()
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device="cuda")   # noqa: E731
    f32 = lambda n: torch.full((n,), -7.0, dtype=torch.float32, device="cuda")   # noqa: E731
    pops, nn_idx, nn_d2, hd_idx, hd_d2 = i32(MAX_BATCH), i32(MAX_BATCH), f32(MAX_BATCH), i32(MAX_BATCH), f32(MAX_BATCH)
    perm_q, perm_r = i32(MAX_BATCH), i32(N_REF)
    order = lambda *a: f("order_dev")(h, *a[:1 if narrow else 0], *a[1:], None)   # noqa: E731  (which: the narrow kind's alone)
    a_need = lib.dc_hip_assign_workspace_bytes(N_REF, MAX_BATCH)
    a_ws = torch.empty(a_need, dtype=torch.uint8, device="cuda")

    def assign(states_ref=states, max_pop=5, r=radius, ws_bytes=a_need):
        a = ctypes.c_void_p(0x1234)
        rc = getattr(lib, assign_open)(h, ptr(states_ref), max_pop, r, ptr(a_ws), ws_bytes, None, ctypes.byref(a))
        assert rc != OK and a.value is None, "refused, and *out is NULL"
        return rc

    try:
        note("stage 9 rows", f("stage_dev")(h, ptr(Q), MAX_BATCH + 1, None))
        note("populations before a stage", f("populations_dev")(h, rad(radius), 1, ptr(pops), None))
        note("nearest before a stage", f("nearest_dev")(h, None, ptr(nn_idx), ptr(nn_d2), None, None, None))
        note("order with perm_q before a stage", order(0, ptr(perm_q), ptr(perm_r)))
        note("assign_open before set_free_energies", assign())
        note("stage null rows", f("stage_dev")(h, None, MAX_BATCH, None))
        rc = f("stage_dev")(h, ptr(Q), MAX_BATCH, None)
        assert rc == OK, lib.dc_hip_last_error()
        note("nearest with fe_query before set_free_energies", f("nearest_dev")(h, ptr(fe_q), ptr(nn_idx), ptr(nn_d2), ptr(hd_idx), ptr(hd_d2), None))
        note("populations null radii", f("populations_dev")(h, None, 1, ptr(pops), None))
        note("populations null pops", f("populations_dev")(h, rad(radius), 1, None, None))
        note("nearest null nn_idx", f("nearest_dev")(h, None, None, ptr(nn_d2), None, None, None))
        note("nearest null nn_d2", f("nearest_dev")(h, None, ptr(nn_idx), None, None, None, None))
        note("set_free_energies null", f("set_free_energies_dev")(h, None, None))
        if narrow:
            note("order which=2", order(2, ptr(perm_q), ptr(perm_r)))
            note("radius just above max_radius", f("populations_dev")(h, rad(np.nextafter(np.float32(radius), np.float32(2 * radius))), 1, ptr(pops), None))
        rc = f("set_free_energies_dev")(h, ptr(fe_r), None)
        assert rc == OK, lib.dc_hip_last_error()
        note("nearest null hd_idx", f("nearest_dev")(h, ptr(fe_q), ptr(nn_idx), ptr(nn_d2), None, ptr(hd_d2), None))
        note("nearest null hd_d2", f("nearest_dev")(h, ptr(fe_q), ptr(nn_idx), ptr(nn_d2), ptr(hd_idx), None, None))
        note("assign_open max_pop=0", assign(max_pop=0))
        note("assign_open NaN radius", assign(r=float("nan")))
        if narrow:
            note("assign_open radius above max_radius", assign(r=1.5 * radius))
        note("assign_open null states", assign(states_ref=None))
        note("assign_open workspace one byte short", assign(ws_bytes=a_need - 1))
        note("assign_open max_pop=0, NaN radius, short workspace", assign(max_pop=0, r=float("nan"), ws_bytes=a_need - 1))
        # ... and the handle still serves the batch staged among the refusals
        rc = f("populations_dev")(h, rad(radius), 1, ptr(pops), None)
        assert rc == OK, lib.dc_hip_last_error()
        rc = f("nearest_dev")(h, ptr(fe_q), ptr(nn_idx), ptr(nn_d2), ptr(hd_idx), ptr(hd_d2), None)
        assert rc == OK, lib.dc_hip_last_error()
        torch.cuda.synchronize()
    finally:
        f("close")(h)
    return got, (pops, nn_idx, nn_d2, hd_idx, hd_d2)


def per_call(dens, kind):
    """the same batch through the per-call pruned entry points"""
    radius = KINDS[kind][3]
    R, Q, fe_r, fe_q, _ = (gpu(a) for a in data(kind))
    Q = Q[:MAX_BATCH].contiguous()
    if kind == "narrow":
        pops = dens.calculate_populations_against(Q, R, [radius], variant="cross_pruned")
        return (pops[0],) + tuple(dens.nearest_reference(Q, R, fe_q, fe_r, pruned=True))
    pops = dens.calculate_populations_against_wide_pruned(Q, R, [radius])
    return (pops[0],) + tuple(dens.nearest_reference_wide_pruned(Q, R, fe_q, fe_r))


@pytest.fixture(scope="module")
def lib():
    from clustering_amd import capi
    return capi.lib


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_refusal_is_the_recorded_one_and_leaves_the_handle_usable(lib, kind):
    from clustering_amd import density
    got, last = sequence(lib, kind)
    for step, (rc, msg) in got.items():
        print(kind, step, rc, msg)
    assert len(got) == (22 if kind == "narrow" else 19)
    assert all(rc in (INVALID, WORKSPACE) for rc, _ in got.values()), "every case is an argument refusal"
    assert got == EXPECTED[kind]
    want = per_call(density, kind)
    assert int(last[0].sum()) > 0 and int(last[0].min()) < N_REF, "the radius separates"
    for name, a, b in zip(("pops", "nn_idx", "nn_d2", "hd_idx", "hd_d2"), last, want):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32)), (kind, name)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from clustering_amd import capi
    print("EXPECTED = " + json.dumps({kind: sequence(capi.lib, kind)[0] for kind in KINDS}, indent=1))
    sys.exit(0)


# kind -> {step of sequence(): [status, text]}; recorded, see the head of this file
EXPECTED = {
 "narrow": {
  "stage 9 rows": [
   -1,
   "dc_hip_reference_stage_dev: n_query=9, the reference was opened for batches of at most 8"
  ],
  "populations before a stage": [
   -1,
   "dc_hip_reference_populations_dev: no batch is staged"
  ],
  "nearest before a stage": [
   -1,
   "dc_hip_reference_nearest_dev: no batch is staged"
  ],
  "order with perm_q before a stage": [
   -1,
   "dc_hip_reference_order_dev: no batch is staged"
  ],
  "assign_open before set_free_energies": [
   -1,
   "dc_hip_assign_open_dev: the reference's free energies were never set"
  ],
  "stage null rows": [
   -1,
   "dc_hip_reference_stage_dev: null pointer"
  ],
  "nearest with fe_query before set_free_energies": [
   -1,
   "dc_hip_reference_nearest_dev: d_fe_query given, but the reference's free energies were never set"
  ],
  "populations null radii": [
   -1,
   "dc_hip_reference_populations_dev: null pointer"
  ],
  "populations null pops": [
   -1,
   "dc_hip_reference_populations_dev: null pointer"
  ],
  "nearest null nn_idx": [
   -1,
   "dc_hip_reference_nearest_dev: null pointer"
  ],
  "nearest null nn_d2": [
   -1,
   "dc_hip_reference_nearest_dev: null pointer"
  ],
  "set_free_energies null": [
   -1,
   "dc_hip_reference_set_free_energies_dev: null pointer"
  ],
  "order which=2": [
   -1,
   "dc_hip_reference_order_dev: which=2: 0 the population order, 1 the neighbours'"
  ],
  "radius just above max_radius": [
   -1,
   "dc_hip_reference_populations_dev: radii[0]=1, the reference was opened for radii whose square is at most 1"
  ],
  "nearest null hd_idx": [
   -1,
   "dc_hip_reference_nearest_dev: null pointer"
  ],
  "nearest null hd_d2": [
   -1,
   "dc_hip_reference_nearest_dev: null pointer"
  ],
  "assign_open max_pop=0": [
   -1,
   "dc_hip_assign_open_dev: max_pop must be positive"
  ],
  "assign_open NaN radius": [
   -1,
   "dc_hip_assign_open_dev: radius=nan must be a number >= 0"
  ],
  "assign_open radius above max_radius": [
   -1,
   "dc_hip_assign_open_dev: radius=1.5, the reference was opened for radii whose square is at most 1"
  ],
  "assign_open null states": [
   -1,
   "dc_hip_assign_open_dev: null pointer"
  ],
  "assign_open workspace one byte short": [
   -5,
   "dc_hip_assign_open_dev: workspace of 2048 bytes needed, got 2047"
  ],
  "assign_open max_pop=0, NaN radius, short workspace": [
   -1,
   "dc_hip_assign_open_dev: max_pop must be positive"
  ]
 },
 "wide": {
  "stage 9 rows": [
   -1,
   "dc_hip_reference_wide_stage_dev: n_query=9, the reference was opened for batches of at most 8"
  ],
  "populations before a stage": [
   -1,
   "dc_hip_reference_wide_populations_dev: no batch is staged"
  ],
  "nearest before a stage": [
   -1,
   "dc_hip_reference_wide_nearest_dev: no batch is staged"
  ],
  "order with perm_q before a stage": [
   -1,
   "dc_hip_reference_wide_order_dev: no batch is staged"
  ],
  "assign_open before set_free_energies": [
   -1,
   "dc_hip_assign_open_wide_dev: the reference's free energies were never set"
  ],
  "stage null rows": [
   -1,
   "dc_hip_reference_wide_stage_dev: null pointer"
  ],
  "nearest with fe_query before set_free_energies": [
   -1,
   "dc_hip_reference_wide_nearest_dev: d_fe_query given, but the reference's free energies were never set"
  ],
  "populations null radii": [
   -1,
   "dc_hip_reference_wide_populations_dev: null pointer"
  ],
  "populations null pops": [
   -1,
   "dc_hip_reference_wide_populations_dev: null pointer"
  ],
  "nearest null nn_idx": [
   -1,
   "dc_hip_reference_wide_nearest_dev: null pointer"
  ],
  "nearest null nn_d2": [
   -1,
   "dc_hip_reference_wide_nearest_dev: null pointer"
  ],
  "set_free_energies null": [
   -1,
   "dc_hip_reference_wide_set_free_energies_dev: null pointer"
  ],
  "nearest null hd_idx": [
   -1,
   "dc_hip_reference_wide_nearest_dev: null pointer"
  ],
  "nearest null hd_d2": [
   -1,
   "dc_hip_reference_wide_nearest_dev: null pointer"
  ],
  "assign_open max_pop=0": [
   -1,
   "dc_hip_assign_open_wide_dev: max_pop must be positive"
  ],
  "assign_open NaN radius": [
   -1,
   "dc_hip_assign_open_wide_dev: radius=nan must be a number >= 0"
  ],
  "assign_open null states": [
   -1,
   "dc_hip_assign_open_wide_dev: null pointer"
  ],
  "assign_open workspace one byte short": [
   -5,
   "dc_hip_assign_open_wide_dev: workspace of 2048 bytes needed, got 2047"
  ],
  "assign_open max_pop=0, NaN radius, short workspace": [
   -1,
   "dc_hip_assign_open_wide_dev: max_pop must be positive"
  ]
 }
}
