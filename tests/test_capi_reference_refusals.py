"""CPU: the refusals of the two resident reference handles (dc_hip_reference_*, 1..64 columns; dc_hip_reference_wide_*,
65..256) that need no device, as a table -- which complaint wins when several arguments are wrong, with its status code and
its dc_hip_last_error() text.  Both handles share one struct and one body per step; each kind keeps its own checks of
open's arguments, in its own order, and the table pins both orders, the twelve calls on a null handle, and
dc_hip_assign_open[_wide]_dev on a null reference.

Every call is made with fake non-null pointers that are never dereferenced: only combinations that return before a device
call are in the grid (reaches_device() below leaves the others out).

The expected values were RECORDED from the library of the commit before the handles were folded, not derived from the code
under test:

    DC_LIB_PATH=<that commit's libdcdensity.so> python tests/test_capi_reference_refusals.py

prints the EXPECTED literal near the end of this file; on a machine without a device the recorder also proves the grid: a call
that reached a device call would come back with a HIP status there, and it refuses to write such a row.
(The refusals of a handle's state need an open handle, which needs a device: tests/test_gpu_reference_refusals.py.)"""
import ctypes
import itertools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, TOO_LARGE, WORKSPACE = 0, -1, -4, -5
FAKE = ctypes.c_void_p(64)      # never dereferenced: the argument checks come first
BIG = 1 << 40                   # bytes no layout of the grid needs
COLS = (0, 1, 64, 65, 256, 257)
COUNTS = {"0": 0, "10": 10, "B": 2 ** 32}
RADII = {"r": 0.5, "nan": float("nan"), "neg": -0.5}     # max_radius: the narrow handle alone takes one
NULLS = ("-", "ref", "out", "ref+out")
WORKSPACES = ("none", "short", "full")
KINDS = {"dc_hip_reference_open_dev": ("dc_hip_reference_workspace_bytes", (1, 64), tuple(RADII)),
         "dc_hip_reference_wide_open_dev": ("dc_hip_reference_wide_workspace_bytes", (65, 256), ("r",))}
RADIUS = np.array([0.5], dtype=np.float32)


def _p(null):
    return None if null else FAKE


def faults(name, case):
    """how many arguments of an open call are wrong"""
    cols, n_ref, max_batch, radius, null, ws = case
    lo, hi = KINDS[name][1]
    return (not lo <= cols <= hi) + (n_ref != "10") + (max_batch != "10") + (radius != "r") + ("ref" in null) + ("out" in null) + \
        (ws != "full")


def reaches_device(name, case):
    """True for the call that passes every check and goes on to prepare the reference: not part of the table"""
    return faults(name, case) == 0


def grid(name):
    """the cases of one open entry point: every combination of column count, the two row counts and the kind's radii with
    the pointers given (so every order among the shape checks is pinned), and every combination with at most two faults"""
    for case in itertools.product(COLS, COUNTS, COUNTS, KINDS[name][2], NULLS, WORKSPACES):
        shape_only = case[4] == "-" and case[5] == "full"
        if (shape_only or faults(name, case) <= 2) and not reaches_device(name, case):
            yield case


def case_id(case):
    return ".".join(str(c) for c in case)


def run_open(lib, name, case):
    cols, n_ref, max_batch, radius, null, ws = case
    n_ref, max_batch = COUNTS[n_ref], COUNTS[max_batch]
    need = getattr(lib, KINDS[name][0])(n_ref, cols, max_batch)
    ws_ptr, ws_bytes = {"none": (None, 0), "short": (FAKE, max(need, 1) - 1), "full": (FAKE, BIG)}[ws]
    h = ctypes.c_void_p(0x1234)
    out = None if "out" in null else ctypes.byref(h)
    extra = (RADII[radius],) if name == "dc_hip_reference_open_dev" else ()
    rc = getattr(lib, name)(_p("ref" in null), n_ref, cols, max_batch, *extra, ws_ptr, ws_bytes, None, out)
    assert out is None or h.value is None or rc == OK, "*out is NULL on a refusal"
    return [rc, lib.dc_hip_last_error().decode() if rc else ""]


def no_handle_calls(lib):
    """name -> the call on a null handle (or, for the two assigner opens, a null reference / a null out); others: whether
    the call's other pointers are given"""
    u64, u32 = ctypes.c_uint64(0), ctypes.c_uint32(0)
    rad = RADIUS.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    calls = {}
    for api in ("dc_hip_reference_", "dc_hip_reference_wide_"):
        narrow = api == "dc_hip_reference_"
        third = u32 if narrow else u64
        f = lambda step, api=api: getattr(lib, api + step)   # noqa: E731
        calls[api + "set_free_energies_dev"] = lambda o, f=f: f("set_free_energies_dev")(None, _p(not o), None)
        calls[api + "stage_dev"] = lambda o, f=f: f("stage_dev")(None, _p(not o), 5, None)
        calls[api + "populations_dev"] = lambda o, f=f: f("populations_dev")(None, rad if o else None, 1, _p(not o), None)
        calls[api + "nearest_dev"] = lambda o, f=f: f("nearest_dev")(None, _p(not o), _p(not o), _p(not o), _p(not o), _p(not o), None)
        calls[api + "info_dev"] = lambda o, f=f, third=third: f("info_dev")(
            None, *((ctypes.byref(u64), ctypes.byref(u64), ctypes.byref(third), ctypes.byref(u32), ctypes.byref(u32)) if o else (None,) * 5), None)
        calls[api + "order_dev"] = lambda o, f=f, narrow=narrow: f("order_dev")(None, *((0,) if narrow else ()), _p(not o), _p(not o), None)
    for name in ("dc_hip_assign_open_dev", "dc_hip_assign_open_wide_dev"):
        def assign_open(o, fn=getattr(lib, name), ref=None, out=True):
            h = ctypes.c_void_p(0x1234)
            rc = fn(ref, _p(not o), 7 if o else 0, 0.5 if o else float("nan"), _p(not o), BIG if o else 0, None, ctypes.byref(h) if out else None)
            assert not out or h.value is None, "*out is NULL on a refusal"
            return rc
        calls[name + " (reference)"] = assign_open
        calls[name + " (out)"] = lambda o, g=assign_open: g(o, ref=FAKE, out=False)
        calls[name + " (reference, out)"] = lambda o, g=assign_open: g(o, out=False)
    return calls


def run_no_handle(lib, call, others):
    rc = call(others)
    return [rc, lib.dc_hip_last_error().decode() if rc else ""]


def record(lib):
    table = {}
    for name in KINDS:
        rows = {}
        for case in grid(name):
            rc, msg = run_open(lib, name, case)
            assert rc in (INVALID, TOO_LARGE, WORKSPACE), f"{name} {case_id(case)}: status {rc} ({msg}): the call went on to a device call"
            rows.setdefault(f"{rc} {msg}", []).append(case_id(case))
        table[name] = {k: " ".join(v) for k, v in rows.items()}
    for name, call in no_handle_calls(lib).items():
        rows = {}
        for others in (True, False):
            rc, msg = run_no_handle(lib, call, others)
            assert rc == INVALID, f"{name}: status {rc} ({msg})"
            rows.setdefault(f"{rc} {msg}", []).append("given" if others else "null")
        table[name] = {k: " ".join(v) for k, v in rows.items()}
    return table


def _lib():
    from clustering_amd import capi
    return capi.lib


def test_the_grid_holds_both_opens_the_double_faults_and_the_calls_without_a_handle():
    lib = _lib()
    for name, (_, (lo, hi), radii) in KINDS.items():
        ids = [case_id(c) for c in grid(name)]
        assert len(ids) == len(set(ids)), name
        have = lambda *parts: any(all(p in i.split(".") for p in parts) for i in ids)   # noqa: E731
        for cols in COLS:
            assert have(str(cols), "B", "0") and have(str(cols), "0", "B") and have(str(cols), "10", "10", "-", "short"), (name, cols)
        for r in radii[1:]:
            assert have("257", r) and have(str(lo), "0", r) and have(str(lo), "B", r) and have(str(hi), r, "ref") and have(str(hi), r, "none"), r
        assert have(str(lo), "ref", "short") and have(str(hi), "ref+out") and have(str(hi), "out", "none") and have("0", "out"), name
        assert f"{lo}.10.10.r.-.full" not in ids and f"{hi}.10.10.r.-.full" not in ids, "a call that opens a handle is not part of the table"
    calls = no_handle_calls(lib)
    assert sum(not name.startswith("dc_hip_assign_open") for name in calls) == 12 and len(calls) == 18


def test_every_refusal_is_the_recorded_one():
    lib = _lib()
    calls = no_handle_calls(lib)
    assert sorted(EXPECTED) == sorted(list(KINDS) + list(calls))
    wrong = []
    for name in KINDS:
        want = {case: outcome for outcome, cases in EXPECTED[name].items() for case in cases.split()}
        cases = list(grid(name))
        assert sorted(want) == sorted(case_id(c) for c in cases), name
        for case in cases:
            rc, msg = run_open(lib, name, case)
            if f"{rc} {msg}" != want[case_id(case)]:
                wrong.append((name, case_id(case), f"{rc} {msg}", want[case_id(case)]))
    for name, call in calls.items():
        want = {case: outcome for outcome, cases in EXPECTED[name].items() for case in cases.split()}
        for others in (True, False):
            rc, msg = run_no_handle(lib, call, others)
            if f"{rc} {msg}" != want["given" if others else "null"]:
                wrong.append((name, others, f"{rc} {msg}", want["given" if others else "null"]))
    assert not wrong, "\n".join(f"{n} {c}: got {g!r}, recorded {w!r}" for n, c, g, w in wrong[:40])


@pytest.mark.parametrize("name,case,status,text", [
    # where the two kinds order their checks differently, spelled out (the table holds them too)
    ("dc_hip_reference_open_dev", "64.0.B.r.-.full", TOO_LARGE, "frame ids"),
    ("dc_hip_reference_wide_open_dev", "65.0.B.r.-.full", TOO_LARGE, "frame ids"),
    ("dc_hip_reference_open_dev", "1.0.10.nan.-.full", INVALID, "must be positive"),
    ("dc_hip_reference_open_dev", "1.10.10.nan.ref.full", INVALID, "max_radius=nan"),
    ("dc_hip_reference_open_dev", "65.10.10.neg.-.full", INVALID, "1..64 columns"),
    ("dc_hip_reference_wide_open_dev", "64.B.10.r.-.full", INVALID, "65..256 columns"),
    ("dc_hip_reference_wide_open_dev", "256.10.10.r.ref.none", INVALID, "null pointer"),
    ("dc_hip_reference_open_dev", "64.10.10.r.-.short", WORKSPACE, "bytes needed, got"),
    ("dc_hip_reference_wide_open_dev", "256.10.10.r.ref+out.full", INVALID, "null pointer (out)"),
])
def test_the_orders_spelled_out(name, case, status, text):
    lib = _lib()
    found = [c for c in grid(name) if case_id(c) == case]
    assert len(found) == 1, "the case is part of the grid"
    rc, msg = run_open(lib, name, found[0])
    assert rc == status and text in msg, (rc, msg)
    assert msg.startswith(name + ":"), msg


# entry point (or, for the calls without a handle, the call) -> {"status text": the cases that end so}; recorded, see the
# head of this file
EXPECTED = {
 "dc_hip_assign_open_dev (out)": {
  "-1 dc_hip_assign_open_dev: null pointer (out)": "given null"
 },
 "dc_hip_assign_open_dev (reference)": {
  "-1 dc_hip_assign_open_dev: null pointer (reference)": "given null"
 },
 "dc_hip_assign_open_dev (reference, out)": {
  "-1 dc_hip_assign_open_dev: null pointer (out)": "given null"
 },
 "dc_hip_assign_open_wide_dev (out)": {
  "-1 dc_hip_assign_open_wide_dev: null pointer (out)": "given null"
 },
 "dc_hip_assign_open_wide_dev (reference)": {
  "-1 dc_hip_assign_open_wide_dev: null pointer (reference)": "given null"
 },
 "dc_hip_assign_open_wide_dev (reference, out)": {
  "-1 dc_hip_assign_open_wide_dev: null pointer (out)": "given null"
 },
 "dc_hip_reference_info_dev": {
  "-1 dc_hip_reference_info_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_nearest_dev": {
  "-1 dc_hip_reference_nearest_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_open_dev": {
  "-1 dc_hip_reference_open_dev: max_radius=-0.5 must be a number >= 0": "1.10.10.neg.-.none 1.10.10.neg.-.short 1.10.10.neg.-.full 1.10.10.neg.ref.full 64.10.10.neg.-.none 64.10.10.neg.-.short 64.10.10.neg.-.full 64.10.10.neg.ref.full",
  "-1 dc_hip_reference_open_dev: max_radius=nan must be a number >= 0": "1.10.10.nan.-.none 1.10.10.nan.-.short 1.10.10.nan.-.full 1.10.10.nan.ref.full 64.10.10.nan.-.none 64.10.10.nan.-.short 64.10.10.nan.-.full 64.10.10.nan.ref.full",
  "-1 dc_hip_reference_open_dev: n_cols=0, the resident reference of the pruned cross sweeps takes 1..64 columns": "0.0.0.r.-.full 0.0.0.nan.-.full 0.0.0.neg.-.full 0.0.10.r.-.full 0.0.10.nan.-.full 0.0.10.neg.-.full 0.0.B.r.-.full 0.0.B.nan.-.full 0.0.B.neg.-.full 0.10.0.r.-.full 0.10.0.nan.-.full 0.10.0.neg.-.full 0.10.10.r.-.none 0.10.10.r.-.short 0.10.10.r.-.full 0.10.10.r.ref.full 0.10.10.nan.-.full 0.10.10.neg.-.full 0.10.B.r.-.full 0.10.B.nan.-.full 0.10.B.neg.-.full 0.B.0.r.-.full 0.B.0.nan.-.full 0.B.0.neg.-.full 0.B.10.r.-.full 0.B.10.nan.-.full 0.B.10.neg.-.full 0.B.B.r.-.full 0.B.B.nan.-.full 0.B.B.neg.-.full",
  "-1 dc_hip_reference_open_dev: n_cols=256, the resident reference of the pruned cross sweeps takes 1..64 columns": "256.0.0.r.-.full 256.0.0.nan.-.full 256.0.0.neg.-.full 256.0.10.r.-.full 256.0.10.nan.-.full 256.0.10.neg.-.full 256.0.B.r.-.full 256.0.B.nan.-.full 256.0.B.neg.-.full 256.10.0.r.-.full 256.10.0.nan.-.full 256.10.0.neg.-.full 256.10.10.r.-.none 256.10.10.r.-.short 256.10.10.r.-.full 256.10.10.r.ref.full 256.10.10.nan.-.full 256.10.10.neg.-.full 256.10.B.r.-.full 256.10.B.nan.-.full 256.10.B.neg.-.full 256.B.0.r.-.full 256.B.0.nan.-.full 256.B.0.neg.-.full 256.B.10.r.-.full 256.B.10.nan.-.full 256.B.10.neg.-.full 256.B.B.r.-.full 256.B.B.nan.-.full 256.B.B.neg.-.full",
  "-1 dc_hip_reference_open_dev: n_cols=257, the resident reference of the pruned cross sweeps takes 1..64 columns": "257.0.0.r.-.full 257.0.0.nan.-.full 257.0.0.neg.-.full 257.0.10.r.-.full 257.0.10.nan.-.full 257.0.10.neg.-.full 257.0.B.r.-.full 257.0.B.nan.-.full 257.0.B.neg.-.full 257.10.0.r.-.full 257.10.0.nan.-.full 257.10.0.neg.-.full 257.10.10.r.-.none 257.10.10.r.-.short 257.10.10.r.-.full 257.10.10.r.ref.full 257.10.10.nan.-.full 257.10.10.neg.-.full 257.10.B.r.-.full 257.10.B.nan.-.full 257.10.B.neg.-.full 257.B.0.r.-.full 257.B.0.nan.-.full 257.B.0.neg.-.full 257.B.10.r.-.full 257.B.10.nan.-.full 257.B.10.neg.-.full 257.B.B.r.-.full 257.B.B.nan.-.full 257.B.B.neg.-.full",
  "-1 dc_hip_reference_open_dev: n_cols=65, the resident reference of the pruned cross sweeps takes 1..64 columns": "65.0.0.r.-.full 65.0.0.nan.-.full 65.0.0.neg.-.full 65.0.10.r.-.full 65.0.10.nan.-.full 65.0.10.neg.-.full 65.0.B.r.-.full 65.0.B.nan.-.full 65.0.B.neg.-.full 65.10.0.r.-.full 65.10.0.nan.-.full 65.10.0.neg.-.full 65.10.10.r.-.none 65.10.10.r.-.short 65.10.10.r.-.full 65.10.10.r.ref.full 65.10.10.nan.-.full 65.10.10.neg.-.full 65.10.B.r.-.full 65.10.B.nan.-.full 65.10.B.neg.-.full 65.B.0.r.-.full 65.B.0.nan.-.full 65.B.0.neg.-.full 65.B.10.r.-.full 65.B.10.nan.-.full 65.B.10.neg.-.full 65.B.B.r.-.full 65.B.B.nan.-.full 65.B.B.neg.-.full",
  "-1 dc_hip_reference_open_dev: n_ref=0, max_batch=0 must be positive": "1.0.0.r.-.full 1.0.0.nan.-.full 1.0.0.neg.-.full 64.0.0.r.-.full 64.0.0.nan.-.full 64.0.0.neg.-.full",
  "-1 dc_hip_reference_open_dev: n_ref=0, max_batch=10 must be positive": "1.0.10.r.-.none 1.0.10.r.-.short 1.0.10.r.-.full 1.0.10.r.ref.full 1.0.10.nan.-.full 1.0.10.neg.-.full 64.0.10.r.-.none 64.0.10.r.-.short 64.0.10.r.-.full 64.0.10.r.ref.full 64.0.10.nan.-.full 64.0.10.neg.-.full",
  "-1 dc_hip_reference_open_dev: n_ref=10, max_batch=0 must be positive": "1.10.0.r.-.none 1.10.0.r.-.short 1.10.0.r.-.full 1.10.0.r.ref.full 1.10.0.nan.-.full 1.10.0.neg.-.full 64.10.0.r.-.none 64.10.0.r.-.short 64.10.0.r.-.full 64.10.0.r.ref.full 64.10.0.nan.-.full 64.10.0.neg.-.full",
  "-1 dc_hip_reference_open_dev: null pointer": "1.10.10.r.ref.none 1.10.10.r.ref.short 1.10.10.r.ref.full 64.10.10.r.ref.none 64.10.10.r.ref.short 64.10.10.r.ref.full",
  "-1 dc_hip_reference_open_dev: null pointer (out)": "0.10.10.r.out.full 1.0.10.r.out.full 1.10.0.r.out.full 1.10.10.r.out.none 1.10.10.r.out.short 1.10.10.r.out.full 1.10.10.r.ref+out.full 1.10.10.nan.out.full 1.10.10.neg.out.full 1.10.B.r.out.full 1.B.10.r.out.full 64.0.10.r.out.full 64.10.0.r.out.full 64.10.10.r.out.none 64.10.10.r.out.short 64.10.10.r.out.full 64.10.10.r.ref+out.full 64.10.10.nan.out.full 64.10.10.neg.out.full 64.10.B.r.out.full 64.B.10.r.out.full 65.10.10.r.out.full 256.10.10.r.out.full 257.10.10.r.out.full",
  "-4 dc_hip_reference_open_dev: max_batch=0, n_ref=4294967296: frame ids must fit uint32": "1.B.0.r.-.full 1.B.0.nan.-.full 1.B.0.neg.-.full 64.B.0.r.-.full 64.B.0.nan.-.full 64.B.0.neg.-.full",
  "-4 dc_hip_reference_open_dev: max_batch=10, n_ref=4294967296: frame ids must fit uint32": "1.B.10.r.-.none 1.B.10.r.-.short 1.B.10.r.-.full 1.B.10.r.ref.full 1.B.10.nan.-.full 1.B.10.neg.-.full 64.B.10.r.-.none 64.B.10.r.-.short 64.B.10.r.-.full 64.B.10.r.ref.full 64.B.10.nan.-.full 64.B.10.neg.-.full",
  "-4 dc_hip_reference_open_dev: max_batch=4294967296, n_ref=0: frame ids must fit uint32": "1.0.B.r.-.full 1.0.B.nan.-.full 1.0.B.neg.-.full 64.0.B.r.-.full 64.0.B.nan.-.full 64.0.B.neg.-.full",
  "-4 dc_hip_reference_open_dev: max_batch=4294967296, n_ref=10: frame ids must fit uint32": "1.10.B.r.-.none 1.10.B.r.-.short 1.10.B.r.-.full 1.10.B.r.ref.full 1.10.B.nan.-.full 1.10.B.neg.-.full 64.10.B.r.-.none 64.10.B.r.-.short 64.10.B.r.-.full 64.10.B.r.ref.full 64.10.B.nan.-.full 64.10.B.neg.-.full",
  "-4 dc_hip_reference_open_dev: max_batch=4294967296, n_ref=4294967296: frame ids must fit uint32": "1.B.B.r.-.full 1.B.B.nan.-.full 1.B.B.neg.-.full 64.B.B.r.-.full 64.B.B.nan.-.full 64.B.B.neg.-.full",
  "-5 dc_hip_reference_open_dev: workspace of 15104 bytes needed, got 0": "1.10.10.r.-.none",
  "-5 dc_hip_reference_open_dev: workspace of 15104 bytes needed, got 15103": "1.10.10.r.-.short",
  "-5 dc_hip_reference_open_dev: workspace of 80128 bytes needed, got 0": "64.10.10.r.-.none",
  "-5 dc_hip_reference_open_dev: workspace of 80128 bytes needed, got 80127": "64.10.10.r.-.short"
 },
 "dc_hip_reference_order_dev": {
  "-1 dc_hip_reference_order_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_populations_dev": {
  "-1 dc_hip_reference_populations_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_set_free_energies_dev": {
  "-1 dc_hip_reference_set_free_energies_dev: null pointer": "given null"
 },
 "dc_hip_reference_stage_dev": {
  "-1 dc_hip_reference_stage_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_wide_info_dev": {
  "-1 dc_hip_reference_wide_info_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_wide_nearest_dev": {
  "-1 dc_hip_reference_wide_nearest_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_wide_open_dev": {
  "-1 dc_hip_reference_wide_open_dev: n_cols=0, the wide matrix-core sweeps take 65..256 columns": "0.0.0.r.-.full 0.0.10.r.-.full 0.0.B.r.-.full 0.10.0.r.-.full 0.10.10.r.-.none 0.10.10.r.-.short 0.10.10.r.-.full 0.10.10.r.ref.full 0.10.B.r.-.full 0.B.0.r.-.full 0.B.10.r.-.full 0.B.B.r.-.full",
  "-1 dc_hip_reference_wide_open_dev: n_cols=1, the wide matrix-core sweeps take 65..256 columns": "1.0.0.r.-.full 1.0.10.r.-.full 1.0.B.r.-.full 1.10.0.r.-.full 1.10.10.r.-.none 1.10.10.r.-.short 1.10.10.r.-.full 1.10.10.r.ref.full 1.10.B.r.-.full 1.B.0.r.-.full 1.B.10.r.-.full 1.B.B.r.-.full",
  "-1 dc_hip_reference_wide_open_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.0.r.-.full 257.0.10.r.-.full 257.0.B.r.-.full 257.10.0.r.-.full 257.10.10.r.-.none 257.10.10.r.-.short 257.10.10.r.-.full 257.10.10.r.ref.full 257.10.B.r.-.full 257.B.0.r.-.full 257.B.10.r.-.full 257.B.B.r.-.full",
  "-1 dc_hip_reference_wide_open_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.0.r.-.full 64.0.10.r.-.full 64.0.B.r.-.full 64.10.0.r.-.full 64.10.10.r.-.none 64.10.10.r.-.short 64.10.10.r.-.full 64.10.10.r.ref.full 64.10.B.r.-.full 64.B.0.r.-.full 64.B.10.r.-.full 64.B.B.r.-.full",
  "-1 dc_hip_reference_wide_open_dev: n_ref=0, max_batch=0 must be positive": "65.0.0.r.-.full 256.0.0.r.-.full",
  "-1 dc_hip_reference_wide_open_dev: n_ref=0, max_batch=10 must be positive": "65.0.10.r.-.none 65.0.10.r.-.short 65.0.10.r.-.full 65.0.10.r.ref.full 256.0.10.r.-.none 256.0.10.r.-.short 256.0.10.r.-.full 256.0.10.r.ref.full",
  "-1 dc_hip_reference_wide_open_dev: n_ref=10, max_batch=0 must be positive": "65.10.0.r.-.none 65.10.0.r.-.short 65.10.0.r.-.full 65.10.0.r.ref.full 256.10.0.r.-.none 256.10.0.r.-.short 256.10.0.r.-.full 256.10.0.r.ref.full",
  "-1 dc_hip_reference_wide_open_dev: null pointer": "65.10.10.r.ref.none 65.10.10.r.ref.short 65.10.10.r.ref.full 256.10.10.r.ref.none 256.10.10.r.ref.short 256.10.10.r.ref.full",
  "-1 dc_hip_reference_wide_open_dev: null pointer (out)": "0.10.10.r.out.full 1.10.10.r.out.full 64.10.10.r.out.full 65.0.10.r.out.full 65.10.0.r.out.full 65.10.10.r.out.none 65.10.10.r.out.short 65.10.10.r.out.full 65.10.10.r.ref+out.full 65.10.B.r.out.full 65.B.10.r.out.full 256.0.10.r.out.full 256.10.0.r.out.full 256.10.10.r.out.none 256.10.10.r.out.short 256.10.10.r.out.full 256.10.10.r.ref+out.full 256.10.B.r.out.full 256.B.10.r.out.full 257.10.10.r.out.full",
  "-4 dc_hip_reference_wide_open_dev: n_query=0, n_ref=4294967296: frame ids must fit uint32": "65.B.0.r.-.full 256.B.0.r.-.full",
  "-4 dc_hip_reference_wide_open_dev: n_query=10, n_ref=4294967296: frame ids must fit uint32": "65.B.10.r.-.none 65.B.10.r.-.short 65.B.10.r.-.full 65.B.10.r.ref.full 256.B.10.r.-.none 256.B.10.r.-.short 256.B.10.r.-.full 256.B.10.r.ref.full",
  "-4 dc_hip_reference_wide_open_dev: n_query=4294967296, n_ref=0: frame ids must fit uint32": "65.0.B.r.-.full 256.0.B.r.-.full",
  "-4 dc_hip_reference_wide_open_dev: n_query=4294967296, n_ref=10: frame ids must fit uint32": "65.10.B.r.-.none 65.10.B.r.-.short 65.10.B.r.-.full 65.10.B.r.ref.full 256.10.B.r.-.none 256.10.B.r.-.short 256.10.B.r.-.full 256.10.B.r.ref.full",
  "-4 dc_hip_reference_wide_open_dev: n_query=4294967296, n_ref=4294967296: frame ids must fit uint32": "65.B.B.r.-.full 256.B.B.r.-.full",
  "-5 dc_hip_reference_wide_open_dev: workspace of 123136 bytes needed, got 0": "65.10.10.r.-.none",
  "-5 dc_hip_reference_wide_open_dev: workspace of 123136 bytes needed, got 123135": "65.10.10.r.-.short",
  "-5 dc_hip_reference_wide_open_dev: workspace of 432896 bytes needed, got 0": "256.10.10.r.-.none",
  "-5 dc_hip_reference_wide_open_dev: workspace of 432896 bytes needed, got 432895": "256.10.10.r.-.short"
 },
 "dc_hip_reference_wide_order_dev": {
  "-1 dc_hip_reference_wide_order_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_wide_populations_dev": {
  "-1 dc_hip_reference_wide_populations_dev: null pointer (reference)": "given null"
 },
 "dc_hip_reference_wide_set_free_energies_dev": {
  "-1 dc_hip_reference_wide_set_free_energies_dev: null pointer": "given null"
 },
 "dc_hip_reference_wide_stage_dev": {
  "-1 dc_hip_reference_wide_stage_dev: null pointer (reference)": "given null"
 }
}


def drive(program):
    """the grid through a stand-alone program (tests/cpp/reference_refusals_main.cpp: the host code under sanitizers,
    no Python in its process) against the recorded table; -> the number of rows, all equal"""
    import subprocess
    rows, want = [], []
    for name in KINDS:
        outcome = {case: o for o, cases in EXPECTED[name].items() for case in cases.split()}
        for case in grid(name):
            cols, n_ref, max_batch, radius, null, ws = case
            rows.append(f"open {name} {cols} {COUNTS[n_ref]} {COUNTS[max_batch]} {RADII[radius]} {int('ref' not in null)} {int('out' not in null)} {ws}")
            want.append(outcome[case_id(case)])
    for name in EXPECTED:
        if name not in KINDS:
            for o, cases in EXPECTED[name].items():
                for others in cases.split():
                    rows.append(f"call {name} {int(others == 'given')}")
                    want.append(o)
    r = subprocess.run([program], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-4000:])
    got = r.stdout.splitlines()
    assert got == want, [(a, b, c) for a, b, c in zip(rows, got, want) if b != c][:20]
    return len(got)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[1:2] == ["--drive"]:
        print(drive(sys.argv[2]), "rows through", sys.argv[2], "equal the recorded table; nothing on its stderr")
    else:
        print("EXPECTED = " + json.dumps(record(_lib()), indent=1, sort_keys=True))
