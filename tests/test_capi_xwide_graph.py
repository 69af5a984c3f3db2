"""CPU: the ten entry points of the radius graph and the neighbour blocks at 257..1024 columns -- they are
in the header, the library and the binding, and they refuse what their 65..256 namesakes refuse, with the same codes,
before a device is touched.  Every call is made with fake non-null pointers that are never dereferenced (the forest: real
host arrays), and only calls that return before a device call are made: this module runs without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import xwidegraphref as xg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, TOO_LARGE, WORKSPACE = 0, -1, -4, -5
FAKE = ctypes.c_void_p(64)      # never dereferenced: the argument checks come first
BIG = 1 << 40
MIN_EDGE_MAX_ROWS = (1 << 24) - 64 * 512   # dc_mfma.hpp kMinEdgeMaxRows: unchanged at these widths
GRAPH = ("dc_hip_radius_pairs_xwide_dev", "dc_hip_radius_min_edge_xwide_dev", "dc_hip_radius_forest_xwide",
         "dc_hip_radius_pairs_xwide_pruned_dev", "dc_hip_radius_min_edge_xwide_pruned_dev", "dc_hip_radius_forest_xwide_pruned")
BLOCKS = ("dc_hip_neighbors_block_rows_xwide", "dc_hip_neighbors_block_pack_xwide_dev", "dc_hip_neighbors_block_unpack_xwide_dev",
          "dc_hip_xwide_layout_status_dev")
OUTSIDE = (0, 64, 65, 256, 1025, 4096)
INSIDE = (257, 300, 401, 1024)


@pytest.fixture(scope="module")
def capi():
    from clustering_amd import capi
    return capi


def last_error(capi):
    return capi.lib.dc_hip_last_error().decode()


def namesake(name):
    return name.replace("_xwide", "_wide")


# ---- the calls: (n_rows, n_cols, segment, n_segments, workspace, bytes, null pointer name or None) -> status -------------
def _p(null, name):
    return None if null == name else FAKE


def call(lib, name, n, d, seg=0, n_seg=0, ws=FAKE, ws_bytes=BIG, null=None):
    fn = getattr(lib, name)
    if "radius_pairs" in name:
        return fn(_p(null, "coords"), n, d, 0.5, _p(null, "pops"), FAKE, 4, _p(null, "count"), ws, ws_bytes, None)
    if "min_edge" in name:
        return fn(_p(null, "coords"), n, d, 0.5, _p(null, "comp"), _p(null, "rank"), seg, n_seg, _p(null, "best"), _p(null, "pops"),
                  ws, ws_bytes, None)
    if "block_pack" in name:
        return fn(_p(null, "nn_idx"), FAKE, FAKE, FAKE, n, d, seg, n_seg, ws, ws_bytes, _p(null, "block"), None)
    assert "block_unpack" in name
    return fn(_p(null, "blocks"), n, d, n_seg, ws, ws_bytes, _p(null, "nn_idx"), FAKE, FAKE, FAKE, None)


DEV = tuple(n for n in GRAPH + BLOCKS if n.endswith("_dev") and "status" not in n)


def good_segment(name):
    """a (segment, n_segments) the call takes"""
    return (1, 3) if "block" in name else (0, 0)


def need(lib, name, n, d):
    pruned = "pruned" in name or "block" in name
    return int((lib.dc_hip_xwide_pruned_workspace_bytes if pruned else lib.dc_hip_xwide_workspace_bytes)(n, d, 1))


# ---- header, library, binding -------------------------------------------------------------------------------------------
def test_the_ten_symbols_are_in_the_header_the_library_and_the_binding(capi):
    header = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    declared = set(re.findall(r"DC_API\s+[\w\s\*]+?\b(dc_hip_\w+)\s*\(", header))
    assert len(GRAPH + BLOCKS) == 10
    for name in GRAPH + BLOCKS:
        assert name in declared, f"{name} is not declared in include/dc_density.h"
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
        fn = getattr(capi.lib, name)
        wide = getattr(capi.lib, namesake(name))
        assert fn.argtypes == wide.argtypes and fn.restype == wide.restype, f"{name}: the argument list of its namesake"
    assert capi.lib.dc_hip_abi_version() == 5, "additive: ABI 5"


def test_the_python_functions_exist_and_refuse_other_widths():
    from clustering_amd import density
    for name in ("radius_pairs_xwide", "radius_min_edge_xwide", "radius_forest_xwide", "radius_pairs_xwide_pruned",
                 "radius_min_edge_xwide_pruned", "radius_forest_xwide_pruned", "neighbor_block_rows_xwide",
                 "pack_neighbor_block_xwide", "unpack_neighbor_blocks_xwide", "xwide_layout_status"):
        assert callable(getattr(density, name)), name
    rank = np.arange(3, dtype=np.uint32)
    for fn in (density.radius_forest_xwide, density.radius_forest_xwide_pruned):
        for d in (256, 1025):
            with pytest.raises(ValueError, match="257..1024"):
                fn(np.zeros((3, d), dtype=np.float32), 1.0, rank)
    for fn in (density.radius_forest_wide, density.radius_forest_wide_pruned):   # (the namesakes keep their own widths)
        with pytest.raises(ValueError, match="65..256"):
            fn(np.zeros((3, 257), dtype=np.float32), 1.0, rank)
    assert density.neighbor_block_rows_xwide(300, 300, 2) == 288 and density.neighbor_block_rows_xwide(300, 256, 2) == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEV)
@pytest.mark.parametrize("n_cols", [256, 1025, 64, 0])
def test_column_counts_outside_the_family_are_invalid_arguments(capi, name, n_cols):
    seg, n_seg = good_segment(name)
    assert call(capi.lib, name, 300, n_cols, seg, n_seg) == INVALID
    msg = last_error(capi)
    assert msg.startswith(name + ":") and "257..1024" in msg and f"n_cols={n_cols}" in msg, msg
    # ... the code of the call it mirrors, one column outside ITS family
    assert call(capi.lib, namesake(name), 300, 64 if n_cols <= 256 else 257, seg, n_seg) == INVALID
    assert last_error(capi).startswith(namesake(name) + ":") and "65..256" in last_error(capi)


@pytest.mark.parametrize("name", DEV)
@pytest.mark.parametrize("n_cols", INSIDE)
def test_a_short_and_a_null_workspace(capi, name, n_cols):
    seg, n_seg = good_segment(name)
    want = need(capi.lib, name, 300, n_cols)
    assert want > 13312, "the layout of these widths: the images start at byte 13 312"
    for ws, ws_bytes in ((None, BIG), (None, 0), (FAKE, want - 1), (FAKE, 0)):
        assert call(capi.lib, name, 300, n_cols, seg, n_seg, ws, ws_bytes) == WORKSPACE, (ws, ws_bytes)
        msg = last_error(capi)
        assert msg.startswith(name + ":") and f"workspace of {want} bytes needed" in msg, msg
    # the workspace of the other family is 0 at these widths and never serves: the namesake refuses the width itself
    assert capi.lib.dc_hip_wide_pruned_workspace_bytes(300, n_cols, 1) == 0 and capi.lib.dc_hip_wide_workspace_bytes(300, n_cols, 1) == 0
    assert call(capi.lib, namesake(name), 300, n_cols, seg, n_seg) == INVALID


@pytest.mark.parametrize("name", DEV)
def test_the_order_of_the_checks_is_that_of_the_namesake(capi, name):
    """per call a list of wrong arguments, each with everything after it in the namesake's order of checks wrong as well:
    the same code from both families, each naming itself"""
    seg, n_seg = good_segment(name)
    nulls = {"radius_pairs": ("count", "coords", "pops"), "min_edge": ("coords", "comp", "rank", "best", "pops"),
             "block_pack": ("nn_idx", "block"), "block_unpack": ("blocks", "nn_idx")}
    nulls = next(v for k, v in nulls.items() if k in name)
    cases = [dict(n=2 ** 32, ws=None), dict(n=300, null=nulls[0], ws=None), dict(n=300, null=nulls[-1], ws=None)]
    if "radius_pairs" not in name and "block_unpack" not in name:   # (the calls that take a segment: checked before the rows)
        cases += [dict(n=300, seg=3, n_seg=3, ws=None, null=nulls[0]), dict(n=0, seg=3, n_seg=3)]
    if "block" in name:
        cases += [dict(n=300, seg=0, n_seg=0, ws=None), dict(n=300, seg=0, n_seg=2 ** 32, ws=None)]
    if "min_edge" in name:
        cases += [dict(n=MIN_EDGE_MAX_ROWS + 1, ws=None)]
    for case in cases:
        kw = dict(seg=seg, n_seg=n_seg)
        kw.update(case)
        n = kw.pop("n")
        got = call(capi.lib, name, n, 300, **kw)
        msg = last_error(capi)
        want = call(capi.lib, namesake(name), n, 100, **kw)
        wide_msg = last_error(capi)
        assert got == want and got != OK, (case, got, want, msg)
        assert msg.startswith(name + ":") and wide_msg.startswith(namesake(name) + ":"), (msg, wide_msg)
        assert re.sub(r"^\S+", "", msg) == re.sub(r"^\S+", "", wide_msg), "the same complaint"


@pytest.mark.parametrize("name", [n for n in DEV if "min_edge" in n])
def test_the_min_edge_row_limit_is_unchanged(capi, name):
    assert call(capi.lib, name, MIN_EDGE_MAX_ROWS + 1, 300) == INVALID
    msg = last_error(capi)
    assert msg.startswith(name + ":") and f"n_rows <= {MIN_EDGE_MAX_ROWS}" in msg, msg
    # at the limit the complaint is the workspace's: the row count itself is taken (no device is reached: no workspace)
    assert call(capi.lib, name, MIN_EDGE_MAX_ROWS, 300, ws=None) == WORKSPACE
    assert call(capi.lib, name, 300, 300, 3, 3) == INVALID and "segment 3 of 3" in last_error(capi)


@pytest.mark.parametrize("name", [n for n in DEV if "radius_pairs" not in n])
def test_no_rows_is_ok(capi, name):
    seg, n_seg = good_segment(name)
    for d in INSIDE:
        assert call(capi.lib, name, 0, d, seg, n_seg, None, 0, null="coords") == OK
    assert call(capi.lib, name, 0, 256, seg, n_seg, None, 0) == INVALID, "the width is checked first"


@pytest.mark.parametrize("name", [n for n in DEV if "radius_pairs" in n])
def test_pairs_of_no_rows_still_want_their_count(capi, name):
    # (with a count the call zeroes it on the device: not made here)
    assert call(capi.lib, name, 0, 300, null="count") == INVALID and "d_count" in last_error(capi)
    assert call(capi.lib, name, 0, 1025) == INVALID and "n_cols=1025" in last_error(capi)


# ---- the forest ---------------------------------------------------------------------------------------------------------
def forest(lib, name, c, rank, n=None, d=None, n_edges=True):
    n = len(c) if n is None else n
    d = c.shape[1] if d is None else d
    edges = np.full((max(n, 2), 2), 7, dtype=np.uint32)
    found, rounds = ctypes.c_size_t(99), ctypes.c_uint32(99)
    rc = getattr(lib, name)(c.ctypes.data_as(ctypes.c_void_p), n, d, 1.0, rank.ctypes.data_as(ctypes.c_void_p), 0,
                            edges.ctypes.data_as(ctypes.c_void_p), ctypes.byref(found) if n_edges else None, ctypes.byref(rounds))
    return rc, found.value, rounds.value, edges


@pytest.mark.parametrize("name", [n for n in GRAPH if "forest" in n])
def test_forest_refusals_and_trivial_forests(capi, name):
    lib = capi.lib
    c = np.zeros((4, 300), dtype=np.float32)
    ident = np.arange(4, dtype=np.uint32)
    for rank in (np.array([0, 1, 1, 2], dtype=np.uint32), np.array([0, 1, 2, 4], dtype=np.uint32)):
        rc, found, rounds, edges = forest(lib, name, c, rank)
        assert rc == INVALID and found == 0 and rounds == 0 and (edges == 7).all()
        assert last_error(capi) == f"{name}: rank is not a permutation of 0..n_rows-1"
    for d in (256, 1025):
        rc, found, rounds, _ = forest(lib, name, c, ident, d=d)
        assert rc == INVALID and found == 0 and rounds == 0 and "257..1024" in last_error(capi)
    for n in (0, 1):
        rc, found, rounds, edges = forest(lib, name, c, ident, n=n)
        assert rc == OK and found == 0 and rounds == 0 and (edges == 7).all()
    rc, _, _, _ = forest(lib, name, c, ident, n=MIN_EDGE_MAX_ROWS + 1)
    assert rc == INVALID and f"n_rows <= {MIN_EDGE_MAX_ROWS}" in last_error(capi) and last_error(capi).startswith(name + ":")
    rc, _, _, _ = forest(lib, name, c, ident, n_edges=False)
    assert rc == INVALID and "n_edges" in last_error(capi)
    rc, _, _, _ = forest(lib, namesake(name), c, ident)
    assert rc == INVALID and "65..256" in last_error(capi), "the namesake refuses these widths"


# ---- the blocks ---------------------------------------------------------------------------------------------------------
def test_block_rows_match_the_formula_and_are_zero_outside_the_range(capi):
    lib = capi.lib
    for n in (0, 1, 2, 127, 128, 129, 300, 700, 1500, 2100, 70000, 2 ** 24):
        for g in (0, 1, 2, 3, 5, 8, 1000):
            for d in INSIDE:
                assert lib.dc_hip_neighbors_block_rows_xwide(n, d, g) == xg.block_rows(n, g), (n, d, g)
            for d in OUTSIDE:
                assert lib.dc_hip_neighbors_block_rows_xwide(n, d, g) == 0, (n, d, g)
            assert lib.dc_hip_neighbors_block_rows_wide(n, 100, g) == xg.block_rows(n, g), "a block is no function of the width"
            assert lib.dc_hip_neighbors_block_rows_wide(n, 257, g) == 0


def test_layout_status_refuses_null_arguments(capi):
    bad = ctypes.c_int(5)
    assert capi.lib.dc_hip_xwide_layout_status_dev(None, ctypes.byref(bad), None) == INVALID
    assert last_error(capi) == "dc_hip_xwide_layout_status_dev: null argument" and bad.value == 5
    assert capi.lib.dc_hip_xwide_layout_status_dev(FAKE, None, None) == INVALID
    assert capi.lib.dc_hip_wide_layout_status_dev(None, ctypes.byref(bad), None) == INVALID
    assert last_error(capi) == "dc_hip_wide_layout_status_dev: null argument"
