"""CPU: the refusals of the wide (65..256 columns) entry points, as a table -- which complaint wins when several arguments
are wrong, with its status code and its dc_hip_last_error() text.  The twelve entry points of the six unpruned / pruned
pairs share one body per pair; the table pins the order of checks of each of them, and of the two block entry points.

Every call is made with fake non-null pointers that are never dereferenced: only combinations that return before a device
call are in the grid (reaches_device() below leaves the others out).

The expected values were RECORDED from the library of the commit before the bodies were folded, not derived from the code
under test:

    DC_LIB_PATH=<that commit's libdcdensity.so> python tests/test_capi_wide_refusals.py

prints the EXPECTED literal at the end of this file; on a machine without a device the recorder also proves the grid: a call that reached a device call would
come back with a HIP status there, and it refuses to write such a row."""
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
N_REF = 10
COLS = (64, 100, 257)
ROWS = {"0": 0, "10": 10, "B": 2 ** 32}
RADII = np.array([0.5], dtype=np.float32)


def _radii(null):
    return None if null else RADII.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _p(null):
    return None if null else FAKE


# entry point -> (its pointers, what it takes besides the shape: a row range, a segment, a segment that must be one, a
# segment count, or nothing; the workspace size function and whether it takes two row counts; the call)
def _entries(lib):
    def size(fn, cross):
        return (lambda n, d: fn(n, N_REF, d, 1)) if cross else (lambda n, d: fn(n, d, 1))

    wide, pruned = size(lib.dc_hip_wide_workspace_bytes, False), size(lib.dc_hip_wide_pruned_workspace_bytes, False)
    cross, cross_pruned = size(lib.dc_hip_cross_wide_workspace_bytes, True), size(lib.dc_hip_cross_wide_pruned_workspace_bytes, True)
    E = {}

    def pop(fn):
        return lambda n, d, a, b, z, ws, wb: fn(_p(z == "coords"), n, d, _radii(z == "radii"), 1, a, b, _p(z == "pops"), ws, wb, None)

    def nn(fn):
        return lambda n, d, a, b, z, ws, wb: fn(_p(z == "coords"), n, d, _p(z == "fe"), a, b, _p(z == "nn_idx"), _p(z == "nn_d2"),
                                                _p(z == "hd_idx"), _p(z == "hd_d2"), ws, wb, None)

    def pairs(fn):
        return lambda n, d, a, b, z, ws, wb: fn(_p(z == "coords"), n, d, 0.5, _p(z == "pops"), FAKE, 4, _p(z == "count"), ws, wb, None)

    def edge(fn):
        return lambda n, d, a, b, z, ws, wb: fn(_p(z == "coords"), n, d, 0.5, _p(z == "comp"), _p(z == "rank"), a, b, _p(z == "best"),
                                                _p(z == "pops"), ws, wb, None)

    def xpop(fn):
        return lambda n, d, a, b, z, ws, wb: fn(_p(z == "query"), n, _p(z == "ref"), N_REF, d, _radii(z == "radii"), 1, a, b,
                                                _p(z == "pops"), ws, wb, None)

    def xnn(fn):
        return lambda n, d, a, b, z, ws, wb: fn(_p(z == "query"), n, _p(z == "ref"), N_REF, d, FAKE, _p(z == "fe_ref"), a, b,
                                                _p(z == "nn_idx"), _p(z == "nn_d2"), _p(z == "hd_idx"), _p(z == "hd_d2"), ws, wb, None)

    nn_ptrs = ("coords", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2")
    edge_ptrs = ("coords", "comp", "rank", "best", "pops")
    xnn_ptrs = ("query", "ref", "fe_ref", "nn_idx", "nn_d2", "hd_idx", "hd_d2")
    E["dc_hip_populations_wide_dev"] = (("coords", "radii", "pops"), "range", wide, pop(lib.dc_hip_populations_wide_dev))
    E["dc_hip_populations_wide_pruned_dev"] = (("coords", "radii", "pops"), "segment", pruned, pop(lib.dc_hip_populations_wide_pruned_dev))
    E["dc_hip_nearest_neighbors_wide_dev"] = (nn_ptrs, "range", wide, nn(lib.dc_hip_nearest_neighbors_wide_dev))
    E["dc_hip_nearest_neighbors_wide_pruned_dev"] = (nn_ptrs, "segment", pruned, nn(lib.dc_hip_nearest_neighbors_wide_pruned_dev))
    E["dc_hip_radius_pairs_wide_dev"] = (("coords", "pops", "count"), None, wide, pairs(lib.dc_hip_radius_pairs_wide_dev))
    E["dc_hip_radius_pairs_wide_pruned_dev"] = (("coords", "pops", "count"), None, pruned, pairs(lib.dc_hip_radius_pairs_wide_pruned_dev))
    E["dc_hip_radius_min_edge_wide_dev"] = (edge_ptrs, "segment", wide, edge(lib.dc_hip_radius_min_edge_wide_dev))
    E["dc_hip_radius_min_edge_wide_pruned_dev"] = (edge_ptrs, "segment", pruned, edge(lib.dc_hip_radius_min_edge_wide_pruned_dev))
    E["dc_hip_populations_cross_wide_dev"] = (("query", "ref", "radii", "pops"), "range", cross, xpop(lib.dc_hip_populations_cross_wide_dev))
    E["dc_hip_populations_cross_wide_pruned_dev"] = (("query", "ref", "radii", "pops"), "range", cross_pruned,
                                                     xpop(lib.dc_hip_populations_cross_wide_pruned_dev))
    E["dc_hip_nearest_neighbors_cross_wide_dev"] = (xnn_ptrs, "range", cross, xnn(lib.dc_hip_nearest_neighbors_cross_wide_dev))
    E["dc_hip_nearest_neighbors_cross_wide_pruned_dev"] = (xnn_ptrs, "range", cross_pruned,
                                                           xnn(lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev))
    E["dc_hip_neighbors_block_pack_wide_dev"] = (
        ("nn_idx", "nn_d2", "hd_idx", "hd_d2", "block"), "segment of some", pruned,
        lambda n, d, a, b, z, ws, wb: lib.dc_hip_neighbors_block_pack_wide_dev(
            _p(z == "nn_idx"), _p(z == "nn_d2"), _p(z == "hd_idx"), _p(z == "hd_d2"), n, d, a, b, ws, wb, _p(z == "block"), None))
    E["dc_hip_neighbors_block_unpack_wide_dev"] = (
        ("blocks", "nn_idx", "nn_d2", "hd_idx", "hd_d2"), "segments", pruned,
        lambda n, d, a, b, z, ws, wb: lib.dc_hip_neighbors_block_unpack_wide_dev(
            _p(z == "blocks"), n, d, b, ws, wb, _p(z == "nn_idx"), _p(z == "nn_d2"), _p(z == "hd_idx"), _p(z == "hd_d2"), None))
    return E


def _second(kind, n, good):
    """the row range or the segment of a call: one that is in order, or one that is not"""
    if kind == "range":
        return (0, n) if good else (3, 2)
    if kind == "segments":
        return (0, 3) if good else (0, 0)
    if kind == "segment of some":
        return (1, 3) if good else (0, 0)    # (a segment beyond the segments: the pruned sweeps' cases; here: no segments)
    if kind == "segment":
        return (1, 3) if good else (3, 3)
    return (0, 0)


def reaches_device(name, kind, cols, rows, good, null, ws):
    """True for the combinations that pass every check and go on to a device call: not part of the table"""
    cols_ok = 65 <= cols <= 256
    if "radius_pairs" in name and rows == "0":
        return cols_ok and null != "count"          # no rows: the count is written before the arrays are looked at
    if "cross" in name and rows == "0":
        return cols_ok and good and ws == "full"    # no queries: a workspace that is given reports that nothing was swept
    if rows != "10":
        return False                                # no rows: OK at once; 2^32 rows: refused whatever else holds
    return cols_ok and (good or kind is None) and null == "-" and ws == "full"


def grid(name, ptrs, kind):
    """(case id, n_cols, rows, second argument in order, null pointer, workspace) of one entry point: every combination of
    column count, row count, range / segment and workspace, all pointers given; and at 100 columns each pointer null in
    turn with every combination of the rest"""
    seconds = (True, False) if kind else (True,)
    for cols, rows, good, ws in itertools.product(COLS, ROWS, seconds, ("none", "short", "full")):
        for null in ("-",) + (ptrs if cols == 100 else ()):
            if not reaches_device(name, kind, cols, rows, good, null, ws):
                yield f"{cols}.{rows}.{'ok' if good else 'bad'}.{null}.{ws}", cols, rows, good, null, ws


def run(lib, entry, kind, case):
    _, cols, rows, good, null, ws = case
    n = ROWS[rows]
    ptrs, _, size, call = entry
    need = size(n, cols)
    ws_ptr, ws_bytes = {"none": (None, 0), "short": (FAKE, max(need, 1) - 1), "full": (FAKE, BIG)}[ws]
    a, b = _second(kind, n, good)
    rc = call(n, cols, a, b, null, ws_ptr, ws_bytes)
    return [rc, lib.dc_hip_last_error().decode() if rc else ""]


def record(lib):
    table = {}
    for name, entry in _entries(lib).items():
        rows = {}
        for case in grid(name, entry[0], entry[1]):
            rc, msg = run(lib, entry, entry[1], case)
            assert rc in (OK, INVALID, TOO_LARGE, WORKSPACE), f"{name} {case[0]}: status {rc} ({msg}): the call went on to a device call"
            rows.setdefault(f"{rc} {msg}".strip(), []).append(case[0])
        table[name] = {k: " ".join(v) for k, v in rows.items()}
    return table


def _lib():
    from clustering_amd import capi
    return capi.lib


def test_the_grid_holds_every_entry_point_and_the_double_faults_that_matter():
    lib = _lib()
    entries = _entries(lib)
    assert len(entries) == 14 and sum(name.endswith("_pruned_dev") for name in entries) == 6
    for name, (ptrs, kind, _, _) in entries.items():
        ids = [c[0] for c in grid(name, ptrs, kind)]
        assert len(ids) == len(set(ids)), name
        have = lambda *parts: any(all(p in i.split(".") for p in parts) for i in ids)   # noqa: E731
        assert have("64", "short") and have("257", "none") and have("100", "B"), name
        first = "count" if "radius_pairs" in name else ptrs[0]   # (the pair list writes its count when there are no rows)
        assert have("100", "0", first) and have("100", "10", ptrs[-1], "short"), (name, "a null pointer: with no rows, with a short workspace")
        if kind:
            assert have("64", "bad") and have("100", "bad", ptrs[0]) and have("100", "0", "bad") and have("100", "B", "bad"), name


def test_every_refusal_is_the_recorded_one():
    lib = _lib()
    expected = EXPECTED
    entries = _entries(lib)
    assert sorted(expected) == sorted(entries)
    wrong = []
    for name, entry in entries.items():
        want = {case: outcome for outcome, cases in expected[name].items() for case in cases.split()}
        cases = list(grid(name, entry[0], entry[1]))
        assert sorted(want) == sorted(c[0] for c in cases), name
        for case in cases:
            rc, msg = run(lib, entry, entry[1], case)
            if f"{rc} {msg}".strip() != want[case[0]]:
                wrong.append((name, case[0], f"{rc} {msg}".strip(), want[case[0]]))
    assert not wrong, "\n".join(f"{n} {c}: got {g!r}, recorded {w!r}" for n, c, g, w in wrong[:40])


@pytest.mark.parametrize("name,case,status,text", [
    # the orders that differ between siblings, spelled out (the table holds them too)
    ("dc_hip_populations_wide_pruned_dev", "64.10.bad.-.full", INVALID, "segment 3 of 3"),
    ("dc_hip_nearest_neighbors_wide_pruned_dev", "257.B.bad.-.none", INVALID, "segment 3 of 3"),
    ("dc_hip_radius_min_edge_wide_pruned_dev", "64.10.bad.-.full", INVALID, "65..256"),
    ("dc_hip_radius_min_edge_wide_dev", "100.B.bad.-.full", TOO_LARGE, "frame ids"),
    ("dc_hip_radius_pairs_wide_pruned_dev", "100.0.ok.count.none", INVALID, "d_count"),
    ("dc_hip_populations_wide_dev", "100.0.ok.coords.none", OK, ""),
    ("dc_hip_nearest_neighbors_cross_wide_pruned_dev", "100.10.ok.hd_d2.short", INVALID, "null pointer"),
    ("dc_hip_neighbors_block_pack_wide_dev", "64.10.bad.-.full", INVALID, "segment 0 of 0"),
])
def test_the_orders_that_differ_between_siblings(name, case, status, text):
    lib = _lib()
    entry = _entries(lib)[name]
    found = [c for c in grid(name, entry[0], entry[1]) if c[0] == case]
    assert len(found) == 1, "the case is part of the grid"
    rc, msg = run(lib, entry, entry[1], found[0])
    assert rc == status and text in msg, (rc, msg)
    assert not rc or msg.startswith(name + ":"), msg



# entry point -> {"status text" ("0": OK): the cases of grid() that end so}; recorded, see the head of this file
EXPECTED = {
 "dc_hip_nearest_neighbors_cross_wide_dev": {
  "-1 dc_hip_nearest_neighbors_cross_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_dev: null pointer": "100.10.ok.query.none 100.10.ok.ref.none 100.10.ok.fe_ref.none 100.10.ok.nn_idx.none 100.10.ok.nn_d2.none 100.10.ok.hd_idx.none 100.10.ok.hd_d2.none 100.10.ok.query.short 100.10.ok.ref.short 100.10.ok.fe_ref.short 100.10.ok.nn_idx.short 100.10.ok.nn_d2.short 100.10.ok.hd_idx.short 100.10.ok.hd_d2.short 100.10.ok.query.full 100.10.ok.ref.full 100.10.ok.fe_ref.full 100.10.ok.nn_idx.full 100.10.ok.nn_d2.full 100.10.ok.hd_idx.full 100.10.ok.hd_d2.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_dev: row range [3, 2) outside [0, 0)": "100.0.bad.-.none 100.0.bad.query.none 100.0.bad.ref.none 100.0.bad.fe_ref.none 100.0.bad.nn_idx.none 100.0.bad.nn_d2.none 100.0.bad.hd_idx.none 100.0.bad.hd_d2.none 100.0.bad.-.short 100.0.bad.query.short 100.0.bad.ref.short 100.0.bad.fe_ref.short 100.0.bad.nn_idx.short 100.0.bad.nn_d2.short 100.0.bad.hd_idx.short 100.0.bad.hd_d2.short 100.0.bad.-.full 100.0.bad.query.full 100.0.bad.ref.full 100.0.bad.fe_ref.full 100.0.bad.nn_idx.full 100.0.bad.nn_d2.full 100.0.bad.hd_idx.full 100.0.bad.hd_d2.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_dev: row range [3, 2) outside [0, 10)": "100.10.bad.-.none 100.10.bad.query.none 100.10.bad.ref.none 100.10.bad.fe_ref.none 100.10.bad.nn_idx.none 100.10.bad.nn_d2.none 100.10.bad.hd_idx.none 100.10.bad.hd_d2.none 100.10.bad.-.short 100.10.bad.query.short 100.10.bad.ref.short 100.10.bad.fe_ref.short 100.10.bad.nn_idx.short 100.10.bad.nn_d2.short 100.10.bad.hd_idx.short 100.10.bad.hd_d2.short 100.10.bad.-.full 100.10.bad.query.full 100.10.bad.ref.full 100.10.bad.fe_ref.full 100.10.bad.nn_idx.full 100.10.bad.nn_d2.full 100.10.bad.hd_idx.full 100.10.bad.hd_d2.full",
  "-4 dc_hip_nearest_neighbors_cross_wide_dev: n_query=4294967296, n_ref=10: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.query.none 100.B.ok.ref.none 100.B.ok.fe_ref.none 100.B.ok.nn_idx.none 100.B.ok.nn_d2.none 100.B.ok.hd_idx.none 100.B.ok.hd_d2.none 100.B.ok.-.short 100.B.ok.query.short 100.B.ok.ref.short 100.B.ok.fe_ref.short 100.B.ok.nn_idx.short 100.B.ok.nn_d2.short 100.B.ok.hd_idx.short 100.B.ok.hd_d2.short 100.B.ok.-.full 100.B.ok.query.full 100.B.ok.ref.full 100.B.ok.fe_ref.full 100.B.ok.nn_idx.full 100.B.ok.nn_d2.full 100.B.ok.hd_idx.full 100.B.ok.hd_d2.full 100.B.bad.-.none 100.B.bad.query.none 100.B.bad.ref.none 100.B.bad.fe_ref.none 100.B.bad.nn_idx.none 100.B.bad.nn_d2.none 100.B.bad.hd_idx.none 100.B.bad.hd_d2.none 100.B.bad.-.short 100.B.bad.query.short 100.B.bad.ref.short 100.B.bad.fe_ref.short 100.B.bad.nn_idx.short 100.B.bad.nn_d2.short 100.B.bad.hd_idx.short 100.B.bad.hd_d2.short 100.B.bad.-.full 100.B.bad.query.full 100.B.bad.ref.full 100.B.bad.fe_ref.full 100.B.bad.nn_idx.full 100.B.bad.nn_d2.full 100.B.bad.hd_idx.full 100.B.bad.hd_d2.full",
  "-5 dc_hip_nearest_neighbors_cross_wide_dev: workspace of 160512 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_nearest_neighbors_cross_wide_dev: workspace of 160512 bytes needed, got 160511": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.query.none 100.0.ok.ref.none 100.0.ok.fe_ref.none 100.0.ok.nn_idx.none 100.0.ok.nn_d2.none 100.0.ok.hd_idx.none 100.0.ok.hd_d2.none 100.0.ok.-.short 100.0.ok.query.short 100.0.ok.ref.short 100.0.ok.fe_ref.short 100.0.ok.nn_idx.short 100.0.ok.nn_d2.short 100.0.ok.hd_idx.short 100.0.ok.hd_d2.short"
 },
 "dc_hip_nearest_neighbors_cross_wide_pruned_dev": {
  "-1 dc_hip_nearest_neighbors_cross_wide_pruned_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_pruned_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_pruned_dev: null pointer": "100.10.ok.query.none 100.10.ok.ref.none 100.10.ok.fe_ref.none 100.10.ok.nn_idx.none 100.10.ok.nn_d2.none 100.10.ok.hd_idx.none 100.10.ok.hd_d2.none 100.10.ok.query.short 100.10.ok.ref.short 100.10.ok.fe_ref.short 100.10.ok.nn_idx.short 100.10.ok.nn_d2.short 100.10.ok.hd_idx.short 100.10.ok.hd_d2.short 100.10.ok.query.full 100.10.ok.ref.full 100.10.ok.fe_ref.full 100.10.ok.nn_idx.full 100.10.ok.nn_d2.full 100.10.ok.hd_idx.full 100.10.ok.hd_d2.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_pruned_dev: row range [3, 2) outside [0, 0)": "100.0.bad.-.none 100.0.bad.query.none 100.0.bad.ref.none 100.0.bad.fe_ref.none 100.0.bad.nn_idx.none 100.0.bad.nn_d2.none 100.0.bad.hd_idx.none 100.0.bad.hd_d2.none 100.0.bad.-.short 100.0.bad.query.short 100.0.bad.ref.short 100.0.bad.fe_ref.short 100.0.bad.nn_idx.short 100.0.bad.nn_d2.short 100.0.bad.hd_idx.short 100.0.bad.hd_d2.short 100.0.bad.-.full 100.0.bad.query.full 100.0.bad.ref.full 100.0.bad.fe_ref.full 100.0.bad.nn_idx.full 100.0.bad.nn_d2.full 100.0.bad.hd_idx.full 100.0.bad.hd_d2.full",
  "-1 dc_hip_nearest_neighbors_cross_wide_pruned_dev: row range [3, 2) outside [0, 10)": "100.10.bad.-.none 100.10.bad.query.none 100.10.bad.ref.none 100.10.bad.fe_ref.none 100.10.bad.nn_idx.none 100.10.bad.nn_d2.none 100.10.bad.hd_idx.none 100.10.bad.hd_d2.none 100.10.bad.-.short 100.10.bad.query.short 100.10.bad.ref.short 100.10.bad.fe_ref.short 100.10.bad.nn_idx.short 100.10.bad.nn_d2.short 100.10.bad.hd_idx.short 100.10.bad.hd_d2.short 100.10.bad.-.full 100.10.bad.query.full 100.10.bad.ref.full 100.10.bad.fe_ref.full 100.10.bad.nn_idx.full 100.10.bad.nn_d2.full 100.10.bad.hd_idx.full 100.10.bad.hd_d2.full",
  "-4 dc_hip_nearest_neighbors_cross_wide_pruned_dev: n_query=4294967296, n_ref=10: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.query.none 100.B.ok.ref.none 100.B.ok.fe_ref.none 100.B.ok.nn_idx.none 100.B.ok.nn_d2.none 100.B.ok.hd_idx.none 100.B.ok.hd_d2.none 100.B.ok.-.short 100.B.ok.query.short 100.B.ok.ref.short 100.B.ok.fe_ref.short 100.B.ok.nn_idx.short 100.B.ok.nn_d2.short 100.B.ok.hd_idx.short 100.B.ok.hd_d2.short 100.B.ok.-.full 100.B.ok.query.full 100.B.ok.ref.full 100.B.ok.fe_ref.full 100.B.ok.nn_idx.full 100.B.ok.nn_d2.full 100.B.ok.hd_idx.full 100.B.ok.hd_d2.full 100.B.bad.-.none 100.B.bad.query.none 100.B.bad.ref.none 100.B.bad.fe_ref.none 100.B.bad.nn_idx.none 100.B.bad.nn_d2.none 100.B.bad.hd_idx.none 100.B.bad.hd_d2.none 100.B.bad.-.short 100.B.bad.query.short 100.B.bad.ref.short 100.B.bad.fe_ref.short 100.B.bad.nn_idx.short 100.B.bad.nn_d2.short 100.B.bad.hd_idx.short 100.B.bad.hd_d2.short 100.B.bad.-.full 100.B.bad.query.full 100.B.bad.ref.full 100.B.bad.fe_ref.full 100.B.bad.nn_idx.full 100.B.bad.nn_d2.full 100.B.bad.hd_idx.full 100.B.bad.hd_d2.full",
  "-5 dc_hip_nearest_neighbors_cross_wide_pruned_dev: workspace of 173568 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_nearest_neighbors_cross_wide_pruned_dev: workspace of 173568 bytes needed, got 173567": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.query.none 100.0.ok.ref.none 100.0.ok.fe_ref.none 100.0.ok.nn_idx.none 100.0.ok.nn_d2.none 100.0.ok.hd_idx.none 100.0.ok.hd_d2.none 100.0.ok.-.short 100.0.ok.query.short 100.0.ok.ref.short 100.0.ok.fe_ref.short 100.0.ok.nn_idx.short 100.0.ok.nn_d2.short 100.0.ok.hd_idx.short 100.0.ok.hd_d2.short"
 },
 "dc_hip_nearest_neighbors_wide_dev": {
  "-1 dc_hip_nearest_neighbors_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_nearest_neighbors_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_nearest_neighbors_wide_dev: null pointer": "100.10.ok.coords.none 100.10.ok.fe.none 100.10.ok.nn_idx.none 100.10.ok.nn_d2.none 100.10.ok.hd_idx.none 100.10.ok.hd_d2.none 100.10.ok.coords.short 100.10.ok.fe.short 100.10.ok.nn_idx.short 100.10.ok.nn_d2.short 100.10.ok.hd_idx.short 100.10.ok.hd_d2.short 100.10.ok.coords.full 100.10.ok.fe.full 100.10.ok.nn_idx.full 100.10.ok.nn_d2.full 100.10.ok.hd_idx.full 100.10.ok.hd_d2.full",
  "-1 dc_hip_nearest_neighbors_wide_dev: row range [3, 2) outside [0, 0)": "100.0.bad.-.none 100.0.bad.coords.none 100.0.bad.fe.none 100.0.bad.nn_idx.none 100.0.bad.nn_d2.none 100.0.bad.hd_idx.none 100.0.bad.hd_d2.none 100.0.bad.-.short 100.0.bad.coords.short 100.0.bad.fe.short 100.0.bad.nn_idx.short 100.0.bad.nn_d2.short 100.0.bad.hd_idx.short 100.0.bad.hd_d2.short 100.0.bad.-.full 100.0.bad.coords.full 100.0.bad.fe.full 100.0.bad.nn_idx.full 100.0.bad.nn_d2.full 100.0.bad.hd_idx.full 100.0.bad.hd_d2.full",
  "-1 dc_hip_nearest_neighbors_wide_dev: row range [3, 2) outside [0, 10)": "100.10.bad.-.none 100.10.bad.coords.none 100.10.bad.fe.none 100.10.bad.nn_idx.none 100.10.bad.nn_d2.none 100.10.bad.hd_idx.none 100.10.bad.hd_d2.none 100.10.bad.-.short 100.10.bad.coords.short 100.10.bad.fe.short 100.10.bad.nn_idx.short 100.10.bad.nn_d2.short 100.10.bad.hd_idx.short 100.10.bad.hd_d2.short 100.10.bad.-.full 100.10.bad.coords.full 100.10.bad.fe.full 100.10.bad.nn_idx.full 100.10.bad.nn_d2.full 100.10.bad.hd_idx.full 100.10.bad.hd_d2.full",
  "-4 dc_hip_nearest_neighbors_wide_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.fe.none 100.B.ok.nn_idx.none 100.B.ok.nn_d2.none 100.B.ok.hd_idx.none 100.B.ok.hd_d2.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.fe.short 100.B.ok.nn_idx.short 100.B.ok.nn_d2.short 100.B.ok.hd_idx.short 100.B.ok.hd_d2.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.fe.full 100.B.ok.nn_idx.full 100.B.ok.nn_d2.full 100.B.ok.hd_idx.full 100.B.ok.hd_d2.full 100.B.bad.-.none 100.B.bad.coords.none 100.B.bad.fe.none 100.B.bad.nn_idx.none 100.B.bad.nn_d2.none 100.B.bad.hd_idx.none 100.B.bad.hd_d2.none 100.B.bad.-.short 100.B.bad.coords.short 100.B.bad.fe.short 100.B.bad.nn_idx.short 100.B.bad.nn_d2.short 100.B.bad.hd_idx.short 100.B.bad.hd_d2.short 100.B.bad.-.full 100.B.bad.coords.full 100.B.bad.fe.full 100.B.bad.nn_idx.full 100.B.bad.nn_d2.full 100.B.bad.hd_idx.full 100.B.bad.hd_d2.full",
  "-5 dc_hip_nearest_neighbors_wide_dev: workspace of 160512 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_nearest_neighbors_wide_dev: workspace of 160512 bytes needed, got 160511": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.coords.none 100.0.ok.fe.none 100.0.ok.nn_idx.none 100.0.ok.nn_d2.none 100.0.ok.hd_idx.none 100.0.ok.hd_d2.none 100.0.ok.-.short 100.0.ok.coords.short 100.0.ok.fe.short 100.0.ok.nn_idx.short 100.0.ok.nn_d2.short 100.0.ok.hd_idx.short 100.0.ok.hd_d2.short 100.0.ok.-.full 100.0.ok.coords.full 100.0.ok.fe.full 100.0.ok.nn_idx.full 100.0.ok.nn_d2.full 100.0.ok.hd_idx.full 100.0.ok.hd_d2.full"
 },
 "dc_hip_nearest_neighbors_wide_pruned_dev": {
  "-1 dc_hip_nearest_neighbors_wide_pruned_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full",
  "-1 dc_hip_nearest_neighbors_wide_pruned_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full",
  "-1 dc_hip_nearest_neighbors_wide_pruned_dev: null pointer": "100.10.ok.coords.none 100.10.ok.fe.none 100.10.ok.nn_idx.none 100.10.ok.nn_d2.none 100.10.ok.hd_idx.none 100.10.ok.hd_d2.none 100.10.ok.coords.short 100.10.ok.fe.short 100.10.ok.nn_idx.short 100.10.ok.nn_d2.short 100.10.ok.hd_idx.short 100.10.ok.hd_d2.short 100.10.ok.coords.full 100.10.ok.fe.full 100.10.ok.nn_idx.full 100.10.ok.nn_d2.full 100.10.ok.hd_idx.full 100.10.ok.hd_d2.full",
  "-1 dc_hip_nearest_neighbors_wide_pruned_dev: segment 3 of 3": "64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full 100.0.bad.-.none 100.0.bad.coords.none 100.0.bad.fe.none 100.0.bad.nn_idx.none 100.0.bad.nn_d2.none 100.0.bad.hd_idx.none 100.0.bad.hd_d2.none 100.0.bad.-.short 100.0.bad.coords.short 100.0.bad.fe.short 100.0.bad.nn_idx.short 100.0.bad.nn_d2.short 100.0.bad.hd_idx.short 100.0.bad.hd_d2.short 100.0.bad.-.full 100.0.bad.coords.full 100.0.bad.fe.full 100.0.bad.nn_idx.full 100.0.bad.nn_d2.full 100.0.bad.hd_idx.full 100.0.bad.hd_d2.full 100.10.bad.-.none 100.10.bad.coords.none 100.10.bad.fe.none 100.10.bad.nn_idx.none 100.10.bad.nn_d2.none 100.10.bad.hd_idx.none 100.10.bad.hd_d2.none 100.10.bad.-.short 100.10.bad.coords.short 100.10.bad.fe.short 100.10.bad.nn_idx.short 100.10.bad.nn_d2.short 100.10.bad.hd_idx.short 100.10.bad.hd_d2.short 100.10.bad.-.full 100.10.bad.coords.full 100.10.bad.fe.full 100.10.bad.nn_idx.full 100.10.bad.nn_d2.full 100.10.bad.hd_idx.full 100.10.bad.hd_d2.full 100.B.bad.-.none 100.B.bad.coords.none 100.B.bad.fe.none 100.B.bad.nn_idx.none 100.B.bad.nn_d2.none 100.B.bad.hd_idx.none 100.B.bad.hd_d2.none 100.B.bad.-.short 100.B.bad.coords.short 100.B.bad.fe.short 100.B.bad.nn_idx.short 100.B.bad.nn_d2.short 100.B.bad.hd_idx.short 100.B.bad.hd_d2.short 100.B.bad.-.full 100.B.bad.coords.full 100.B.bad.fe.full 100.B.bad.nn_idx.full 100.B.bad.nn_d2.full 100.B.bad.hd_idx.full 100.B.bad.hd_d2.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-4 dc_hip_nearest_neighbors_wide_pruned_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.fe.none 100.B.ok.nn_idx.none 100.B.ok.nn_d2.none 100.B.ok.hd_idx.none 100.B.ok.hd_d2.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.fe.short 100.B.ok.nn_idx.short 100.B.ok.nn_d2.short 100.B.ok.hd_idx.short 100.B.ok.hd_d2.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.fe.full 100.B.ok.nn_idx.full 100.B.ok.nn_d2.full 100.B.ok.hd_idx.full 100.B.ok.hd_d2.full",
  "-5 dc_hip_nearest_neighbors_wide_pruned_dev: workspace of 168960 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_nearest_neighbors_wide_pruned_dev: workspace of 168960 bytes needed, got 168959": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.coords.none 100.0.ok.fe.none 100.0.ok.nn_idx.none 100.0.ok.nn_d2.none 100.0.ok.hd_idx.none 100.0.ok.hd_d2.none 100.0.ok.-.short 100.0.ok.coords.short 100.0.ok.fe.short 100.0.ok.nn_idx.short 100.0.ok.nn_d2.short 100.0.ok.hd_idx.short 100.0.ok.hd_d2.short 100.0.ok.-.full 100.0.ok.coords.full 100.0.ok.fe.full 100.0.ok.nn_idx.full 100.0.ok.nn_d2.full 100.0.ok.hd_idx.full 100.0.ok.hd_d2.full"
 },
 "dc_hip_neighbors_block_pack_wide_dev": {
  "-1 dc_hip_neighbors_block_pack_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full",
  "-1 dc_hip_neighbors_block_pack_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full",
  "-1 dc_hip_neighbors_block_pack_wide_dev: null pointer": "100.10.ok.nn_idx.none 100.10.ok.nn_d2.none 100.10.ok.hd_idx.none 100.10.ok.hd_d2.none 100.10.ok.block.none 100.10.ok.nn_idx.short 100.10.ok.nn_d2.short 100.10.ok.hd_idx.short 100.10.ok.hd_d2.short 100.10.ok.block.short 100.10.ok.nn_idx.full 100.10.ok.nn_d2.full 100.10.ok.hd_idx.full 100.10.ok.hd_d2.full 100.10.ok.block.full",
  "-1 dc_hip_neighbors_block_pack_wide_dev: segment 0 of 0": "64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full 100.0.bad.-.none 100.0.bad.nn_idx.none 100.0.bad.nn_d2.none 100.0.bad.hd_idx.none 100.0.bad.hd_d2.none 100.0.bad.block.none 100.0.bad.-.short 100.0.bad.nn_idx.short 100.0.bad.nn_d2.short 100.0.bad.hd_idx.short 100.0.bad.hd_d2.short 100.0.bad.block.short 100.0.bad.-.full 100.0.bad.nn_idx.full 100.0.bad.nn_d2.full 100.0.bad.hd_idx.full 100.0.bad.hd_d2.full 100.0.bad.block.full 100.10.bad.-.none 100.10.bad.nn_idx.none 100.10.bad.nn_d2.none 100.10.bad.hd_idx.none 100.10.bad.hd_d2.none 100.10.bad.block.none 100.10.bad.-.short 100.10.bad.nn_idx.short 100.10.bad.nn_d2.short 100.10.bad.hd_idx.short 100.10.bad.hd_d2.short 100.10.bad.block.short 100.10.bad.-.full 100.10.bad.nn_idx.full 100.10.bad.nn_d2.full 100.10.bad.hd_idx.full 100.10.bad.hd_d2.full 100.10.bad.block.full 100.B.bad.-.none 100.B.bad.nn_idx.none 100.B.bad.nn_d2.none 100.B.bad.hd_idx.none 100.B.bad.hd_d2.none 100.B.bad.block.none 100.B.bad.-.short 100.B.bad.nn_idx.short 100.B.bad.nn_d2.short 100.B.bad.hd_idx.short 100.B.bad.hd_d2.short 100.B.bad.block.short 100.B.bad.-.full 100.B.bad.nn_idx.full 100.B.bad.nn_d2.full 100.B.bad.hd_idx.full 100.B.bad.hd_d2.full 100.B.bad.block.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-4 dc_hip_neighbors_block_pack_wide_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.nn_idx.none 100.B.ok.nn_d2.none 100.B.ok.hd_idx.none 100.B.ok.hd_d2.none 100.B.ok.block.none 100.B.ok.-.short 100.B.ok.nn_idx.short 100.B.ok.nn_d2.short 100.B.ok.hd_idx.short 100.B.ok.hd_d2.short 100.B.ok.block.short 100.B.ok.-.full 100.B.ok.nn_idx.full 100.B.ok.nn_d2.full 100.B.ok.hd_idx.full 100.B.ok.hd_d2.full 100.B.ok.block.full",
  "-5 dc_hip_neighbors_block_pack_wide_dev: workspace of 168960 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_neighbors_block_pack_wide_dev: workspace of 168960 bytes needed, got 168959": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.nn_idx.none 100.0.ok.nn_d2.none 100.0.ok.hd_idx.none 100.0.ok.hd_d2.none 100.0.ok.block.none 100.0.ok.-.short 100.0.ok.nn_idx.short 100.0.ok.nn_d2.short 100.0.ok.hd_idx.short 100.0.ok.hd_d2.short 100.0.ok.block.short 100.0.ok.-.full 100.0.ok.nn_idx.full 100.0.ok.nn_d2.full 100.0.ok.hd_idx.full 100.0.ok.hd_d2.full 100.0.ok.block.full"
 },
 "dc_hip_neighbors_block_unpack_wide_dev": {
  "-1 dc_hip_neighbors_block_unpack_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full",
  "-1 dc_hip_neighbors_block_unpack_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full",
  "-1 dc_hip_neighbors_block_unpack_wide_dev: n_segments must be positive": "64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full 100.0.bad.-.none 100.0.bad.blocks.none 100.0.bad.nn_idx.none 100.0.bad.nn_d2.none 100.0.bad.hd_idx.none 100.0.bad.hd_d2.none 100.0.bad.-.short 100.0.bad.blocks.short 100.0.bad.nn_idx.short 100.0.bad.nn_d2.short 100.0.bad.hd_idx.short 100.0.bad.hd_d2.short 100.0.bad.-.full 100.0.bad.blocks.full 100.0.bad.nn_idx.full 100.0.bad.nn_d2.full 100.0.bad.hd_idx.full 100.0.bad.hd_d2.full 100.10.bad.-.none 100.10.bad.blocks.none 100.10.bad.nn_idx.none 100.10.bad.nn_d2.none 100.10.bad.hd_idx.none 100.10.bad.hd_d2.none 100.10.bad.-.short 100.10.bad.blocks.short 100.10.bad.nn_idx.short 100.10.bad.nn_d2.short 100.10.bad.hd_idx.short 100.10.bad.hd_d2.short 100.10.bad.-.full 100.10.bad.blocks.full 100.10.bad.nn_idx.full 100.10.bad.nn_d2.full 100.10.bad.hd_idx.full 100.10.bad.hd_d2.full 100.B.bad.-.none 100.B.bad.blocks.none 100.B.bad.nn_idx.none 100.B.bad.nn_d2.none 100.B.bad.hd_idx.none 100.B.bad.hd_d2.none 100.B.bad.-.short 100.B.bad.blocks.short 100.B.bad.nn_idx.short 100.B.bad.nn_d2.short 100.B.bad.hd_idx.short 100.B.bad.hd_d2.short 100.B.bad.-.full 100.B.bad.blocks.full 100.B.bad.nn_idx.full 100.B.bad.nn_d2.full 100.B.bad.hd_idx.full 100.B.bad.hd_d2.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_neighbors_block_unpack_wide_dev: null pointer": "100.10.ok.blocks.none 100.10.ok.nn_idx.none 100.10.ok.nn_d2.none 100.10.ok.hd_idx.none 100.10.ok.hd_d2.none 100.10.ok.blocks.short 100.10.ok.nn_idx.short 100.10.ok.nn_d2.short 100.10.ok.hd_idx.short 100.10.ok.hd_d2.short 100.10.ok.blocks.full 100.10.ok.nn_idx.full 100.10.ok.nn_d2.full 100.10.ok.hd_idx.full 100.10.ok.hd_d2.full",
  "-4 dc_hip_neighbors_block_unpack_wide_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.blocks.none 100.B.ok.nn_idx.none 100.B.ok.nn_d2.none 100.B.ok.hd_idx.none 100.B.ok.hd_d2.none 100.B.ok.-.short 100.B.ok.blocks.short 100.B.ok.nn_idx.short 100.B.ok.nn_d2.short 100.B.ok.hd_idx.short 100.B.ok.hd_d2.short 100.B.ok.-.full 100.B.ok.blocks.full 100.B.ok.nn_idx.full 100.B.ok.nn_d2.full 100.B.ok.hd_idx.full 100.B.ok.hd_d2.full",
  "-5 dc_hip_neighbors_block_unpack_wide_dev: workspace of 168960 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_neighbors_block_unpack_wide_dev: workspace of 168960 bytes needed, got 168959": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.blocks.none 100.0.ok.nn_idx.none 100.0.ok.nn_d2.none 100.0.ok.hd_idx.none 100.0.ok.hd_d2.none 100.0.ok.-.short 100.0.ok.blocks.short 100.0.ok.nn_idx.short 100.0.ok.nn_d2.short 100.0.ok.hd_idx.short 100.0.ok.hd_d2.short 100.0.ok.-.full 100.0.ok.blocks.full 100.0.ok.nn_idx.full 100.0.ok.nn_d2.full 100.0.ok.hd_idx.full 100.0.ok.hd_d2.full"
 },
 "dc_hip_populations_cross_wide_dev": {
  "-1 dc_hip_populations_cross_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_populations_cross_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_populations_cross_wide_dev: null pointer": "100.10.ok.query.none 100.10.ok.ref.none 100.10.ok.radii.none 100.10.ok.pops.none 100.10.ok.query.short 100.10.ok.ref.short 100.10.ok.radii.short 100.10.ok.pops.short 100.10.ok.query.full 100.10.ok.ref.full 100.10.ok.radii.full 100.10.ok.pops.full",
  "-1 dc_hip_populations_cross_wide_dev: row range [3, 2) outside [0, 0)": "100.0.bad.-.none 100.0.bad.query.none 100.0.bad.ref.none 100.0.bad.radii.none 100.0.bad.pops.none 100.0.bad.-.short 100.0.bad.query.short 100.0.bad.ref.short 100.0.bad.radii.short 100.0.bad.pops.short 100.0.bad.-.full 100.0.bad.query.full 100.0.bad.ref.full 100.0.bad.radii.full 100.0.bad.pops.full",
  "-1 dc_hip_populations_cross_wide_dev: row range [3, 2) outside [0, 10)": "100.10.bad.-.none 100.10.bad.query.none 100.10.bad.ref.none 100.10.bad.radii.none 100.10.bad.pops.none 100.10.bad.-.short 100.10.bad.query.short 100.10.bad.ref.short 100.10.bad.radii.short 100.10.bad.pops.short 100.10.bad.-.full 100.10.bad.query.full 100.10.bad.ref.full 100.10.bad.radii.full 100.10.bad.pops.full",
  "-4 dc_hip_populations_cross_wide_dev: n_query=4294967296, n_ref=10: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.query.none 100.B.ok.ref.none 100.B.ok.radii.none 100.B.ok.pops.none 100.B.ok.-.short 100.B.ok.query.short 100.B.ok.ref.short 100.B.ok.radii.short 100.B.ok.pops.short 100.B.ok.-.full 100.B.ok.query.full 100.B.ok.ref.full 100.B.ok.radii.full 100.B.ok.pops.full 100.B.bad.-.none 100.B.bad.query.none 100.B.bad.ref.none 100.B.bad.radii.none 100.B.bad.pops.none 100.B.bad.-.short 100.B.bad.query.short 100.B.bad.ref.short 100.B.bad.radii.short 100.B.bad.pops.short 100.B.bad.-.full 100.B.bad.query.full 100.B.bad.ref.full 100.B.bad.radii.full 100.B.bad.pops.full",
  "-5 dc_hip_populations_cross_wide_dev: workspace of 160512 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_populations_cross_wide_dev: workspace of 160512 bytes needed, got 160511": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.query.none 100.0.ok.ref.none 100.0.ok.radii.none 100.0.ok.pops.none 100.0.ok.-.short 100.0.ok.query.short 100.0.ok.ref.short 100.0.ok.radii.short 100.0.ok.pops.short"
 },
 "dc_hip_populations_cross_wide_pruned_dev": {
  "-1 dc_hip_populations_cross_wide_pruned_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_populations_cross_wide_pruned_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_populations_cross_wide_pruned_dev: null pointer": "100.10.ok.query.none 100.10.ok.ref.none 100.10.ok.radii.none 100.10.ok.pops.none 100.10.ok.query.short 100.10.ok.ref.short 100.10.ok.radii.short 100.10.ok.pops.short 100.10.ok.query.full 100.10.ok.ref.full 100.10.ok.radii.full 100.10.ok.pops.full",
  "-1 dc_hip_populations_cross_wide_pruned_dev: row range [3, 2) outside [0, 0)": "100.0.bad.-.none 100.0.bad.query.none 100.0.bad.ref.none 100.0.bad.radii.none 100.0.bad.pops.none 100.0.bad.-.short 100.0.bad.query.short 100.0.bad.ref.short 100.0.bad.radii.short 100.0.bad.pops.short 100.0.bad.-.full 100.0.bad.query.full 100.0.bad.ref.full 100.0.bad.radii.full 100.0.bad.pops.full",
  "-1 dc_hip_populations_cross_wide_pruned_dev: row range [3, 2) outside [0, 10)": "100.10.bad.-.none 100.10.bad.query.none 100.10.bad.ref.none 100.10.bad.radii.none 100.10.bad.pops.none 100.10.bad.-.short 100.10.bad.query.short 100.10.bad.ref.short 100.10.bad.radii.short 100.10.bad.pops.short 100.10.bad.-.full 100.10.bad.query.full 100.10.bad.ref.full 100.10.bad.radii.full 100.10.bad.pops.full",
  "-4 dc_hip_populations_cross_wide_pruned_dev: n_query=4294967296, n_ref=10: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.query.none 100.B.ok.ref.none 100.B.ok.radii.none 100.B.ok.pops.none 100.B.ok.-.short 100.B.ok.query.short 100.B.ok.ref.short 100.B.ok.radii.short 100.B.ok.pops.short 100.B.ok.-.full 100.B.ok.query.full 100.B.ok.ref.full 100.B.ok.radii.full 100.B.ok.pops.full 100.B.bad.-.none 100.B.bad.query.none 100.B.bad.ref.none 100.B.bad.radii.none 100.B.bad.pops.none 100.B.bad.-.short 100.B.bad.query.short 100.B.bad.ref.short 100.B.bad.radii.short 100.B.bad.pops.short 100.B.bad.-.full 100.B.bad.query.full 100.B.bad.ref.full 100.B.bad.radii.full 100.B.bad.pops.full",
  "-5 dc_hip_populations_cross_wide_pruned_dev: workspace of 173568 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_populations_cross_wide_pruned_dev: workspace of 173568 bytes needed, got 173567": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.query.none 100.0.ok.ref.none 100.0.ok.radii.none 100.0.ok.pops.none 100.0.ok.-.short 100.0.ok.query.short 100.0.ok.ref.short 100.0.ok.radii.short 100.0.ok.pops.short"
 },
 "dc_hip_populations_wide_dev": {
  "-1 dc_hip_populations_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_populations_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_populations_wide_dev: null pointer": "100.10.ok.coords.none 100.10.ok.radii.none 100.10.ok.pops.none 100.10.ok.coords.short 100.10.ok.radii.short 100.10.ok.pops.short 100.10.ok.coords.full 100.10.ok.radii.full 100.10.ok.pops.full",
  "-1 dc_hip_populations_wide_dev: row range [3, 2) outside [0, 0)": "100.0.bad.-.none 100.0.bad.coords.none 100.0.bad.radii.none 100.0.bad.pops.none 100.0.bad.-.short 100.0.bad.coords.short 100.0.bad.radii.short 100.0.bad.pops.short 100.0.bad.-.full 100.0.bad.coords.full 100.0.bad.radii.full 100.0.bad.pops.full",
  "-1 dc_hip_populations_wide_dev: row range [3, 2) outside [0, 10)": "100.10.bad.-.none 100.10.bad.coords.none 100.10.bad.radii.none 100.10.bad.pops.none 100.10.bad.-.short 100.10.bad.coords.short 100.10.bad.radii.short 100.10.bad.pops.short 100.10.bad.-.full 100.10.bad.coords.full 100.10.bad.radii.full 100.10.bad.pops.full",
  "-4 dc_hip_populations_wide_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.radii.none 100.B.ok.pops.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.radii.short 100.B.ok.pops.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.radii.full 100.B.ok.pops.full 100.B.bad.-.none 100.B.bad.coords.none 100.B.bad.radii.none 100.B.bad.pops.none 100.B.bad.-.short 100.B.bad.coords.short 100.B.bad.radii.short 100.B.bad.pops.short 100.B.bad.-.full 100.B.bad.coords.full 100.B.bad.radii.full 100.B.bad.pops.full",
  "-5 dc_hip_populations_wide_dev: workspace of 160512 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_populations_wide_dev: workspace of 160512 bytes needed, got 160511": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.coords.none 100.0.ok.radii.none 100.0.ok.pops.none 100.0.ok.-.short 100.0.ok.coords.short 100.0.ok.radii.short 100.0.ok.pops.short 100.0.ok.-.full 100.0.ok.coords.full 100.0.ok.radii.full 100.0.ok.pops.full"
 },
 "dc_hip_populations_wide_pruned_dev": {
  "-1 dc_hip_populations_wide_pruned_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full",
  "-1 dc_hip_populations_wide_pruned_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full",
  "-1 dc_hip_populations_wide_pruned_dev: null pointer": "100.10.ok.coords.none 100.10.ok.radii.none 100.10.ok.pops.none 100.10.ok.coords.short 100.10.ok.radii.short 100.10.ok.pops.short 100.10.ok.coords.full 100.10.ok.radii.full 100.10.ok.pops.full",
  "-1 dc_hip_populations_wide_pruned_dev: segment 3 of 3": "64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full 100.0.bad.-.none 100.0.bad.coords.none 100.0.bad.radii.none 100.0.bad.pops.none 100.0.bad.-.short 100.0.bad.coords.short 100.0.bad.radii.short 100.0.bad.pops.short 100.0.bad.-.full 100.0.bad.coords.full 100.0.bad.radii.full 100.0.bad.pops.full 100.10.bad.-.none 100.10.bad.coords.none 100.10.bad.radii.none 100.10.bad.pops.none 100.10.bad.-.short 100.10.bad.coords.short 100.10.bad.radii.short 100.10.bad.pops.short 100.10.bad.-.full 100.10.bad.coords.full 100.10.bad.radii.full 100.10.bad.pops.full 100.B.bad.-.none 100.B.bad.coords.none 100.B.bad.radii.none 100.B.bad.pops.none 100.B.bad.-.short 100.B.bad.coords.short 100.B.bad.radii.short 100.B.bad.pops.short 100.B.bad.-.full 100.B.bad.coords.full 100.B.bad.radii.full 100.B.bad.pops.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-4 dc_hip_populations_wide_pruned_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.radii.none 100.B.ok.pops.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.radii.short 100.B.ok.pops.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.radii.full 100.B.ok.pops.full",
  "-5 dc_hip_populations_wide_pruned_dev: workspace of 168960 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_populations_wide_pruned_dev: workspace of 168960 bytes needed, got 168959": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.coords.none 100.0.ok.radii.none 100.0.ok.pops.none 100.0.ok.-.short 100.0.ok.coords.short 100.0.ok.radii.short 100.0.ok.pops.short 100.0.ok.-.full 100.0.ok.coords.full 100.0.ok.radii.full 100.0.ok.pops.full"
 },
 "dc_hip_radius_min_edge_wide_dev": {
  "-1 dc_hip_radius_min_edge_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_radius_min_edge_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_radius_min_edge_wide_dev: null pointer": "100.10.ok.coords.none 100.10.ok.comp.none 100.10.ok.rank.none 100.10.ok.best.none 100.10.ok.pops.none 100.10.ok.coords.short 100.10.ok.comp.short 100.10.ok.rank.short 100.10.ok.best.short 100.10.ok.pops.short 100.10.ok.coords.full 100.10.ok.comp.full 100.10.ok.rank.full 100.10.ok.best.full 100.10.ok.pops.full",
  "-1 dc_hip_radius_min_edge_wide_dev: segment 3 of 3": "100.0.bad.-.none 100.0.bad.coords.none 100.0.bad.comp.none 100.0.bad.rank.none 100.0.bad.best.none 100.0.bad.pops.none 100.0.bad.-.short 100.0.bad.coords.short 100.0.bad.comp.short 100.0.bad.rank.short 100.0.bad.best.short 100.0.bad.pops.short 100.0.bad.-.full 100.0.bad.coords.full 100.0.bad.comp.full 100.0.bad.rank.full 100.0.bad.best.full 100.0.bad.pops.full 100.10.bad.-.none 100.10.bad.coords.none 100.10.bad.comp.none 100.10.bad.rank.none 100.10.bad.best.none 100.10.bad.pops.none 100.10.bad.-.short 100.10.bad.coords.short 100.10.bad.comp.short 100.10.bad.rank.short 100.10.bad.best.short 100.10.bad.pops.short 100.10.bad.-.full 100.10.bad.coords.full 100.10.bad.comp.full 100.10.bad.rank.full 100.10.bad.best.full 100.10.bad.pops.full",
  "-4 dc_hip_radius_min_edge_wide_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.comp.none 100.B.ok.rank.none 100.B.ok.best.none 100.B.ok.pops.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.comp.short 100.B.ok.rank.short 100.B.ok.best.short 100.B.ok.pops.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.comp.full 100.B.ok.rank.full 100.B.ok.best.full 100.B.ok.pops.full 100.B.bad.-.none 100.B.bad.coords.none 100.B.bad.comp.none 100.B.bad.rank.none 100.B.bad.best.none 100.B.bad.pops.none 100.B.bad.-.short 100.B.bad.coords.short 100.B.bad.comp.short 100.B.bad.rank.short 100.B.bad.best.short 100.B.bad.pops.short 100.B.bad.-.full 100.B.bad.coords.full 100.B.bad.comp.full 100.B.bad.rank.full 100.B.bad.best.full 100.B.bad.pops.full",
  "-5 dc_hip_radius_min_edge_wide_dev: workspace of 160512 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_radius_min_edge_wide_dev: workspace of 160512 bytes needed, got 160511": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.coords.none 100.0.ok.comp.none 100.0.ok.rank.none 100.0.ok.best.none 100.0.ok.pops.none 100.0.ok.-.short 100.0.ok.coords.short 100.0.ok.comp.short 100.0.ok.rank.short 100.0.ok.best.short 100.0.ok.pops.short 100.0.ok.-.full 100.0.ok.coords.full 100.0.ok.comp.full 100.0.ok.rank.full 100.0.ok.best.full 100.0.ok.pops.full"
 },
 "dc_hip_radius_min_edge_wide_pruned_dev": {
  "-1 dc_hip_radius_min_edge_wide_pruned_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.0.bad.-.none 257.0.bad.-.short 257.0.bad.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.10.bad.-.none 257.10.bad.-.short 257.10.bad.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full 257.B.bad.-.none 257.B.bad.-.short 257.B.bad.-.full",
  "-1 dc_hip_radius_min_edge_wide_pruned_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.0.bad.-.none 64.0.bad.-.short 64.0.bad.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.10.bad.-.none 64.10.bad.-.short 64.10.bad.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full 64.B.bad.-.none 64.B.bad.-.short 64.B.bad.-.full",
  "-1 dc_hip_radius_min_edge_wide_pruned_dev: null pointer": "100.10.ok.coords.none 100.10.ok.comp.none 100.10.ok.rank.none 100.10.ok.best.none 100.10.ok.pops.none 100.10.ok.coords.short 100.10.ok.comp.short 100.10.ok.rank.short 100.10.ok.best.short 100.10.ok.pops.short 100.10.ok.coords.full 100.10.ok.comp.full 100.10.ok.rank.full 100.10.ok.best.full 100.10.ok.pops.full",
  "-1 dc_hip_radius_min_edge_wide_pruned_dev: segment 3 of 3": "100.0.bad.-.none 100.0.bad.coords.none 100.0.bad.comp.none 100.0.bad.rank.none 100.0.bad.best.none 100.0.bad.pops.none 100.0.bad.-.short 100.0.bad.coords.short 100.0.bad.comp.short 100.0.bad.rank.short 100.0.bad.best.short 100.0.bad.pops.short 100.0.bad.-.full 100.0.bad.coords.full 100.0.bad.comp.full 100.0.bad.rank.full 100.0.bad.best.full 100.0.bad.pops.full 100.10.bad.-.none 100.10.bad.coords.none 100.10.bad.comp.none 100.10.bad.rank.none 100.10.bad.best.none 100.10.bad.pops.none 100.10.bad.-.short 100.10.bad.coords.short 100.10.bad.comp.short 100.10.bad.rank.short 100.10.bad.best.short 100.10.bad.pops.short 100.10.bad.-.full 100.10.bad.coords.full 100.10.bad.comp.full 100.10.bad.rank.full 100.10.bad.best.full 100.10.bad.pops.full",
  "-4 dc_hip_radius_min_edge_wide_pruned_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.comp.none 100.B.ok.rank.none 100.B.ok.best.none 100.B.ok.pops.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.comp.short 100.B.ok.rank.short 100.B.ok.best.short 100.B.ok.pops.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.comp.full 100.B.ok.rank.full 100.B.ok.best.full 100.B.ok.pops.full 100.B.bad.-.none 100.B.bad.coords.none 100.B.bad.comp.none 100.B.bad.rank.none 100.B.bad.best.none 100.B.bad.pops.none 100.B.bad.-.short 100.B.bad.coords.short 100.B.bad.comp.short 100.B.bad.rank.short 100.B.bad.best.short 100.B.bad.pops.short 100.B.bad.-.full 100.B.bad.coords.full 100.B.bad.comp.full 100.B.bad.rank.full 100.B.bad.best.full 100.B.bad.pops.full",
  "-5 dc_hip_radius_min_edge_wide_pruned_dev: workspace of 168960 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_radius_min_edge_wide_pruned_dev: workspace of 168960 bytes needed, got 168959": "100.10.ok.-.short",
  "0": "100.0.ok.-.none 100.0.ok.coords.none 100.0.ok.comp.none 100.0.ok.rank.none 100.0.ok.best.none 100.0.ok.pops.none 100.0.ok.-.short 100.0.ok.coords.short 100.0.ok.comp.short 100.0.ok.rank.short 100.0.ok.best.short 100.0.ok.pops.short 100.0.ok.-.full 100.0.ok.coords.full 100.0.ok.comp.full 100.0.ok.rank.full 100.0.ok.best.full 100.0.ok.pops.full"
 },
 "dc_hip_radius_pairs_wide_dev": {
  "-1 dc_hip_radius_pairs_wide_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full",
  "-1 dc_hip_radius_pairs_wide_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full",
  "-1 dc_hip_radius_pairs_wide_dev: null pointer": "100.10.ok.coords.none 100.10.ok.pops.none 100.10.ok.coords.short 100.10.ok.pops.short 100.10.ok.coords.full 100.10.ok.pops.full",
  "-1 dc_hip_radius_pairs_wide_dev: null pointer (d_count)": "100.0.ok.count.none 100.0.ok.count.short 100.0.ok.count.full 100.10.ok.count.none 100.10.ok.count.short 100.10.ok.count.full",
  "-4 dc_hip_radius_pairs_wide_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.pops.none 100.B.ok.count.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.pops.short 100.B.ok.count.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.pops.full 100.B.ok.count.full",
  "-5 dc_hip_radius_pairs_wide_dev: workspace of 160512 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_radius_pairs_wide_dev: workspace of 160512 bytes needed, got 160511": "100.10.ok.-.short"
 },
 "dc_hip_radius_pairs_wide_pruned_dev": {
  "-1 dc_hip_radius_pairs_wide_pruned_dev: n_cols=257, the wide matrix-core sweeps take 65..256 columns": "257.0.ok.-.none 257.0.ok.-.short 257.0.ok.-.full 257.10.ok.-.none 257.10.ok.-.short 257.10.ok.-.full 257.B.ok.-.none 257.B.ok.-.short 257.B.ok.-.full",
  "-1 dc_hip_radius_pairs_wide_pruned_dev: n_cols=64, the wide matrix-core sweeps take 65..256 columns": "64.0.ok.-.none 64.0.ok.-.short 64.0.ok.-.full 64.10.ok.-.none 64.10.ok.-.short 64.10.ok.-.full 64.B.ok.-.none 64.B.ok.-.short 64.B.ok.-.full",
  "-1 dc_hip_radius_pairs_wide_pruned_dev: null pointer": "100.10.ok.coords.none 100.10.ok.pops.none 100.10.ok.coords.short 100.10.ok.pops.short 100.10.ok.coords.full 100.10.ok.pops.full",
  "-1 dc_hip_radius_pairs_wide_pruned_dev: null pointer (d_count)": "100.0.ok.count.none 100.0.ok.count.short 100.0.ok.count.full 100.10.ok.count.none 100.10.ok.count.short 100.10.ok.count.full",
  "-4 dc_hip_radius_pairs_wide_pruned_dev: n_rows=4294967296: frame ids must fit uint32": "100.B.ok.-.none 100.B.ok.coords.none 100.B.ok.pops.none 100.B.ok.count.none 100.B.ok.-.short 100.B.ok.coords.short 100.B.ok.pops.short 100.B.ok.count.short 100.B.ok.-.full 100.B.ok.coords.full 100.B.ok.pops.full 100.B.ok.count.full",
  "-5 dc_hip_radius_pairs_wide_pruned_dev: workspace of 168960 bytes needed, got 0": "100.10.ok.-.none",
  "-5 dc_hip_radius_pairs_wide_pruned_dev: workspace of 168960 bytes needed, got 168959": "100.10.ok.-.short"
 }
}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print("EXPECTED = " + json.dumps(record(_lib()), indent=1, sort_keys=True))
