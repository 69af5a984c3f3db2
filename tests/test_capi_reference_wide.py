"""CPU: the interface of the resident reference of the pruned wide cross sweeps (dc_hip_reference_wide_*): the nine symbols
are declared, listed, bound and exported by all three builds; the ABI number, the variants and the pinned workspace values
of the pruned cross sweeps stay; every refusal that needs no handle comes back before a device is touched, with fake
pointers that are never dereferenced, naming the function; the workspace query is monotone and zero where it should be.
(The refusals of a handle's state -- a batch beyond max_batch, a sweep before a stage, free energies that were never set --
need an open handle, which needs a device: tests/test_gpu_wide_reference.py.)"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_reference_wide_workspace_bytes", "dc_hip_reference_wide_open_dev", "dc_hip_reference_wide_close",
         "dc_hip_reference_wide_set_free_energies_dev", "dc_hip_reference_wide_stage_dev", "dc_hip_reference_wide_populations_dev",
         "dc_hip_reference_wide_nearest_dev", "dc_hip_reference_wide_info_dev", "dc_hip_reference_wide_order_dev")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
FAKE = 0x10000   # never dereferenced: every call below is refused first


def test_the_symbols_are_declared_listed_and_bound_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in NAMES:
        assert re.search(r"DC_API\s+(int|void|size_t)\s+" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS and getattr(capi.lib, name).argtypes is not None, name
    assert re.search(r"typedef\s+struct\s+dc_reference_wide\s+dc_reference_wide\s*;", text)
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}
    for method in ("stage", "populations", "nearest", "set_free_energies", "info", "order", "close", "assign", "__enter__", "__exit__"):
        assert callable(getattr(density.Reference, method)), method
    for prop in ("n_ref", "n_cols", "max_batch"):
        assert isinstance(getattr(density.Reference, prop), property), prop


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_the_pruned_cross_sweeps_workspace_query_keeps_its_values():
    """the pins of tests/test_capi_cross_wide_nn_pruned.py: the resident form has a layout of its own"""
    from clustering_amd import capi
    f = capi.lib.dc_hip_cross_wide_pruned_workspace_bytes
    pins = {(1, 1, 65): 116992, (5, 3, 100): 168448, (300, 1500, 100): 1953024, (1500, 300, 256): 4972288,
            (1100, 8320, 80): 8166400, (20000, 200000, 100): 228630784}
    for (n_q, n_r, d), want in pins.items():
        assert f(n_q, n_r, d, 1) == want, (n_q, n_r, d)


def test_the_workspace_query_is_monotone_and_zero_where_it_should_be():
    from clustering_amd import capi
    f = capi.lib.dc_hip_reference_wide_workspace_bytes
    sizes = (1, 2, 127, 128, 129, 1000, 1500, 8320, 20000, 200000)
    for d in (0, 1, 64, 257, 1000):
        assert f(1500, d, 300) == 0, d
    for d in (65, 100, 256):
        assert f(0, d, 300) == 0 and f(1500, d, 0) == 0
        for fixed in (1, 300, 20000):
            last_r = last_b = 0
            for n in sizes:
                a, b = f(n, d, fixed), f(fixed, d, n)
                assert a >= last_r > -1 and b >= last_b and a > 0 and b > 0 and a % 256 == 0, (n, d, fixed)
                last_r, last_b = a, b
    for n_r, n_b in ((1500, 300), (200000, 20000)):
        assert f(n_r, 65, n_b) <= f(n_r, 100, n_b) <= f(n_r, 256, n_b), "monotone in the columns"
    # the resident form holds what the pruned cross sweep of the same shape holds, and the free energies it keeps
    assert f(200000, 100, 20000) >= capi.lib.dc_hip_cross_wide_pruned_workspace_bytes(20000, 200000, 100, 1)


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    name = b"dc_hip_reference_wide_open_dev"

    def open_(d_ref=FAKE, n_ref=1500, n_cols=100, max_batch=300, ws=FAKE, ws_bytes=None, out=True):
        h = ctypes.c_void_p(0x1234)
        need = lib.dc_hip_reference_wide_workspace_bytes(n_ref, n_cols, max_batch) if ws_bytes is None else ws_bytes
        rc = lib.dc_hip_reference_wide_open_dev(d_ref, n_ref, n_cols, max_batch, ws, need, None, ctypes.byref(h) if out else None)
        assert rc != 0 and name in lib.dc_hip_last_error(), (rc, lib.dc_hip_last_error())
        assert not out or h.value is None, "*out is NULL on a refusal"
        return rc

    for d in (0, 1, 64, 257):
        assert open_(n_cols=d, ws_bytes=1 << 30) == INVALID, d
    assert open_(n_ref=0, ws_bytes=1 << 30) == INVALID and open_(max_batch=0, ws_bytes=1 << 30) == INVALID
    assert open_(d_ref=None) == INVALID and open_(out=False) == INVALID
    need = lib.dc_hip_reference_wide_workspace_bytes(1500, 100, 300)
    assert open_(ws_bytes=need - 1) == WORKSPACE and open_(ws=None) == WORKSPACE and open_(ws=None, ws_bytes=0) == WORKSPACE
    # a workspace of the pruned cross sweep of the same shape is not enough: the resident form keeps more
    assert open_(ws_bytes=lib.dc_hip_cross_wide_pruned_workspace_bytes(300, 1500, 100, 1)) == WORKSPACE
    # frame ids must fit uint32, and the elements the index arithmetic
    assert open_(n_ref=2 ** 32 - 1, ws_bytes=1 << 30) == TOO_LARGE and open_(max_batch=2 ** 32, ws_bytes=1 << 30) == TOO_LARGE
    assert open_(n_ref=2 ** 32 * 4 // 100 + 1, ws_bytes=1 << 30) == TOO_LARGE
    assert open_(max_batch=2 ** 32 * 4 // 100 + 1, ws_bytes=1 << 30) == TOO_LARGE
    # no handle: every call on one is refused, and close takes a null pointer
    calls = {"dc_hip_reference_wide_set_free_energies_dev": (FAKE,), "dc_hip_reference_wide_stage_dev": (FAKE, 10),
             "dc_hip_reference_wide_populations_dev": (None, 1, FAKE), "dc_hip_reference_wide_nearest_dev": (None, FAKE, FAKE, None, None),
             "dc_hip_reference_wide_info_dev": (None, None, None, None, None), "dc_hip_reference_wide_order_dev": (FAKE, FAKE)}
    for fn, args in calls.items():
        assert getattr(lib, fn)(None, *args, None) == INVALID, fn
        assert fn.encode() in lib.dc_hip_last_error(), fn
    lib.dc_hip_reference_wide_close(None)
