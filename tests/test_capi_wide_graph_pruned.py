"""CPU: the interface of the PRUNED radius graph on the wide matrix-core sweep (65..256 columns): the three entry points
are declared, listed, bound and exported by all three builds, the ABI number and the variant table stay, and every
refusal comes back before a device is touched -- the device pointers are never valid -- with the codes of the calls they
mirror, naming the function.  (dc_hip_radius_pairs_wide_pruned_dev with no rows writes its count, so that one call is made
on the device: tests/test_gpu_wide_graph_pruned.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_radius_pairs_wide_pruned_dev", "dc_hip_radius_min_edge_wide_pruned_dev", "dc_hip_radius_forest_wide_pruned")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
BIG = 1 << 30
FAKE = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first


def test_the_symbols_are_declared_listed_and_bound_and_the_abi_number_stays():
    from clustering_amd import capi
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in NAMES:
        assert re.search(r"DC_API\s+int\s+" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS and hasattr(capi.lib, name), name
        assert getattr(capi.lib, name).restype is ctypes.c_int, name
        assert getattr(capi.lib, name).argtypes == getattr(capi.lib, name.replace("_pruned", "")).argtypes, name
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def calls():
    from clustering_amd import capi
    lib = capi.lib
    rank = np.arange(10, dtype=np.uint32)
    edges = np.zeros((9, 2), dtype=np.uint32)
    n_edges, n_rounds = ctypes.c_size_t(7), ctypes.c_uint32(7)

    def pairs(n=10, d=100, coords=FAKE, pops=FAKE, count=FAKE, ws=FAKE, ws_bytes=BIG):
        return lib.dc_hip_radius_pairs_wide_pruned_dev(coords, n, d, 0.5, pops, FAKE, 4, count, ws, ws_bytes, None)

    def edge(n=10, d=100, segment=0, n_segments=0, coords=FAKE, comp=FAKE, ws=FAKE, ws_bytes=BIG):
        return lib.dc_hip_radius_min_edge_wide_pruned_dev(coords, n, d, 0.5, comp, FAKE, segment, n_segments, FAKE, FAKE, ws,
                                                          ws_bytes, None)

    def forest(n=10, d=100, rank=rank, coords=FAKE, device=0):
        n_edges.value, n_rounds.value = 7, 7
        rc = lib.dc_hip_radius_forest_wide_pruned(coords, n, d, 0.5, rank.ctypes.data_as(ctypes.c_void_p), device,
                                                  edges.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_edges),
                                                  ctypes.byref(n_rounds))
        assert n_edges.value == 0 and n_rounds.value == 0, "a refused or empty call reports no pair and no round"
        return rc
    return lib, pairs, edge, forest


def test_refusals_come_before_a_device_is_touched():
    lib, pairs, edge, forest = calls()
    for call, name in zip((pairs, edge, forest), NAMES):
        for d in (64, 257, 0, 10, 400):
            assert call(d=d) == INVALID, (name, d)
            assert name.encode() + b":" in lib.dc_hip_last_error() and b"65..256" in lib.dc_hip_last_error(), (name, d)
        assert call(n=2 ** 32) == TOO_LARGE and name.encode() + b":" in lib.dc_hip_last_error(), name
    # a workspace one byte short, the unpruned sweeps' workspace (too small for the order), and none at all
    need = lib.dc_hip_wide_pruned_workspace_bytes(10, 100, 1)
    assert need > lib.dc_hip_wide_workspace_bytes(10, 100, 1) > 0
    for call, name in ((pairs, NAMES[0]), (edge, NAMES[1])):
        assert call(ws_bytes=need - 1) == WORKSPACE and name.encode() + b":" in lib.dc_hip_last_error()
        assert call(ws_bytes=lib.dc_hip_wide_workspace_bytes(10, 100, 1)) == WORKSPACE
        assert call(n=1000, ws_bytes=lib.dc_hip_wide_workspace_bytes(1000, 100, 1)) == WORKSPACE
        assert call(ws=None, ws_bytes=0) == WORKSPACE
        assert call(ws=None, ws_bytes=BIG) == WORKSPACE
        assert call(coords=None) == INVALID
    # the pair list: the count is not optional
    assert pairs(count=None) == INVALID and b"d_count" in lib.dc_hip_last_error()
    assert pairs(pops=None) == INVALID
    # the round: a segment beyond the segments, a null array, more rows than the call it mirrors takes
    for segment, n_segments in ((1, 1), (3, 3), (7, 2), (2 ** 40, 5)):
        assert edge(segment=segment, n_segments=n_segments) == INVALID and b"segment" in lib.dc_hip_last_error()
    assert edge(comp=None) == INVALID
    limit = 2 ** 24 - 32768
    assert edge(n=limit + 1) == INVALID and b"n_rows <=" in lib.dc_hip_last_error()
    assert edge(n=limit, ws=None, ws_bytes=0) == WORKSPACE, "the row limit itself passes that check"
    # the forest: a rank that is no permutation (a value twice; a value beyond the rows), null arrays, the row limit
    for bad in (np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8], dtype=np.uint32), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 10], dtype=np.uint32)):
        assert forest(rank=bad) == INVALID and b"permutation" in lib.dc_hip_last_error()
        assert NAMES[2].encode() + b":" in lib.dc_hip_last_error()
    assert forest(coords=None) == INVALID
    assert forest(n=limit + 1) == INVALID and b"n_rows <=" in lib.dc_hip_last_error()
    assert lib.dc_hip_radius_forest_wide_pruned(FAKE, 10, 100, 0.5, FAKE, 0, FAKE, None, None) == INVALID
    assert b"n_edges" in lib.dc_hip_last_error()


def test_calls_with_no_rows_return_ok():
    lib, pairs, edge, forest = calls()
    for d in (65, 256):
        assert edge(n=0, d=d, coords=None, comp=None, ws=None, ws_bytes=0) == 0
        assert edge(n=0, d=d, segment=2, n_segments=3, coords=None, comp=None, ws=None, ws_bytes=0) == 0
        assert forest(n=0, d=d, coords=None) == 0
        assert forest(n=1, d=d, coords=None) == 0, "one frame: no pair, no sweep"
    # ... but not at another width
    assert edge(n=0, d=64, coords=None, comp=None, ws=None, ws_bytes=0) == INVALID
    assert forest(n=0, d=257, coords=None) == INVALID


def test_the_python_functions_exist_and_refuse_other_column_counts():
    import inspect

    import torch
    from clustering_amd import density
    for name in ("radius_pairs_wide", "radius_min_edge_wide", "radius_forest_wide"):
        assert list(inspect.signature(getattr(density, name + "_pruned")).parameters) == \
            list(inspect.signature(getattr(density, name)).parameters), name
        assert inspect.signature(getattr(density, name + "_pruned")).parameters.keys() == \
            inspect.signature(getattr(density, name.replace("_wide", ""))).parameters.keys(), name
    for d in (10, 64, 257, 400):
        t = torch.zeros((4, d))
        i = torch.zeros(4, dtype=torch.int32)
        with pytest.raises(ValueError, match="65..256"):
            density.radius_pairs_wide_pruned(t, 1.0)
        with pytest.raises(ValueError, match="65..256"):
            density.radius_min_edge_wide_pruned(t, 1.0, i, i)
        with pytest.raises(ValueError, match="65..256"):
            density.radius_forest_wide_pruned(np.zeros((4, d), dtype=np.float32), 1.0, np.arange(4))
