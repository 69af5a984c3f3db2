"""CPU: the interface of the resident reference of the pruned cross sweeps for rows of 1..64 columns (dc_hip_reference_*):
the nine symbols are declared, listed, bound and exported by all three builds; the ABI number and the variants stay; every
refusal that needs no handle comes back before a device is touched, with fake pointers that are never dereferenced, naming
the function; the workspace query is monotone and zero where it should be.
(The refusals of a handle's state -- a batch beyond max_batch, a sweep before a stage, free energies that were never set, a
radius beyond max_radius -- need an open handle, which needs a device: tests/test_gpu_reference.py.)"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_reference_workspace_bytes", "dc_hip_reference_open_dev", "dc_hip_reference_close",
         "dc_hip_reference_set_free_energies_dev", "dc_hip_reference_stage_dev", "dc_hip_reference_populations_dev",
         "dc_hip_reference_nearest_dev", "dc_hip_reference_info_dev", "dc_hip_reference_order_dev")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
FAKE = 0x10000   # never dereferenced: every call below is refused first


def test_the_symbols_are_declared_listed_and_bound_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in NAMES:
        assert re.search(r"DC_API\s+(int|void|size_t)\s+" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS and getattr(capi.lib, name).argtypes is not None, name
    assert re.search(r"typedef\s+struct\s+dc_reference\s+dc_reference\s*;", text)
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}
    for method in ("stage", "populations", "nearest", "set_free_energies", "info", "order", "close", "assign", "__enter__", "__exit__"):
        assert callable(getattr(density.NarrowReference, method)), method
    for prop in ("n_ref", "n_cols", "max_batch"):
        assert isinstance(getattr(density.NarrowReference, prop), property), prop


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_the_workspace_query_is_monotone_and_zero_where_it_should_be():
    from clustering_amd import capi
    f = capi.lib.dc_hip_reference_workspace_bytes
    sizes = (1, 2, 31, 32, 33, 1000, 1500, 8320, 100000, 1000000)
    for d in (0, 65, 100, 256, 1000):
        assert f(1500, d, 300) == 0, d
    for d in (1, 2, 10, 30, 64):
        assert f(0, d, 300) == 0 and f(1500, d, 0) == 0
        for fixed in (1, 300, 20000):
            last_r = last_b = 0
            for n in sizes:
                a, b = f(n, d, fixed), f(fixed, d, n)
                assert a >= last_r and b >= last_b and a > 0 and b > 0 and a % 256 == 0, (n, d, fixed)
                last_r, last_b = a, b
    for n_r, n_b in ((1500, 300), (1000000, 100000)):
        last = 0
        for d in range(1, 65):
            assert f(n_r, d, n_b) >= last, "monotone in the columns"
            last = f(n_r, d, n_b)
    # the resident form holds what both per-call sweeps of the same shape hold of the reference, side by side
    assert f(1000000, 10, 100000) >= capi.lib.dc_hip_nearest_cross_pruned_workspace_bytes(100000, 1000000, 10)


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    name = b"dc_hip_reference_open_dev"

    def open_(d_ref=FAKE, n_ref=1500, n_cols=10, max_batch=300, max_radius=0.5, ws=FAKE, ws_bytes=None, out=True):
        h = ctypes.c_void_p(0x1234)
        need = lib.dc_hip_reference_workspace_bytes(n_ref, n_cols, max_batch) if ws_bytes is None else ws_bytes
        rc = lib.dc_hip_reference_open_dev(d_ref, n_ref, n_cols, max_batch, max_radius, ws, need, None, ctypes.byref(h) if out else None)
        assert rc != 0 and name in lib.dc_hip_last_error(), (rc, lib.dc_hip_last_error())
        assert not out or h.value is None, "*out is NULL on a refusal"
        return rc

    for d in (0, 65, 100, 257):
        assert open_(n_cols=d, ws_bytes=1 << 30) == INVALID, d
    assert open_(n_ref=0, ws_bytes=1 << 30) == INVALID and open_(max_batch=0, ws_bytes=1 << 30) == INVALID
    assert open_(d_ref=None) == INVALID and open_(out=False) == INVALID
    for bad in (float("nan"), -0.5, float("-inf")):
        assert open_(max_radius=bad) == INVALID, bad
    need = lib.dc_hip_reference_workspace_bytes(1500, 10, 300)
    assert open_(ws_bytes=need - 1) == WORKSPACE and open_(ws=None) == WORKSPACE and open_(ws=None, ws_bytes=0) == WORKSPACE
    # a workspace of one per-call pruned sweep of the same shape is not enough: the resident form keeps the reference twice
    assert open_(ws_bytes=lib.dc_hip_nearest_cross_pruned_workspace_bytes(300, 1500, 10)) == WORKSPACE
    # frame ids must fit uint32, and the elements the index arithmetic
    assert open_(n_ref=2 ** 32 - 1, ws_bytes=1 << 30) == TOO_LARGE and open_(max_batch=2 ** 32, ws_bytes=1 << 30) == TOO_LARGE
    assert open_(n_ref=2 ** 32 * 4 // 10 + 1, ws_bytes=1 << 30) == TOO_LARGE
    assert open_(max_batch=2 ** 32 * 4 // 10 + 1, ws_bytes=1 << 30) == TOO_LARGE
    # a reference whose padded order exceeds 2^24 positions: the band-pair queue cannot address it
    assert open_(n_ref=2 ** 24 + 1, n_cols=1, ws_bytes=1 << 40) == TOO_LARGE
    assert b"2^24" in lib.dc_hip_last_error()
    assert lib.dc_hip_reference_workspace_bytes(2 ** 24, 1, 300) > 0
    # no handle: every call on one is refused, and close takes a null pointer
    calls = {"dc_hip_reference_set_free_energies_dev": (FAKE,), "dc_hip_reference_stage_dev": (FAKE, 10),
             "dc_hip_reference_populations_dev": (None, 1, FAKE), "dc_hip_reference_nearest_dev": (None, FAKE, FAKE, None, None),
             "dc_hip_reference_info_dev": (None, None, None, None, None), "dc_hip_reference_order_dev": (0, FAKE, FAKE)}
    for fn, args in calls.items():
        assert getattr(lib, fn)(None, *args, None) == INVALID, fn
        assert fn.encode() in lib.dc_hip_last_error(), fn
    lib.dc_hip_reference_close(None)


def test_the_wide_handle_keeps_refusing_these_widths():
    from clustering_amd import capi
    h = ctypes.c_void_p(0x1234)
    rc = capi.lib.dc_hip_reference_wide_open_dev(FAKE, 1500, 10, 300, FAKE, 1 << 30, None, ctypes.byref(h))
    assert rc == INVALID and h.value is None
    assert capi.lib.dc_hip_reference_wide_workspace_bytes(1500, 10, 300) == 0
