"""CPU: the interface of the pruned neighbour sweep against a reference: its three entry points are declared, listed and
exported by all three builds, the ABI number stays, the workspace query follows its rule, and the argument refusals come
back before a device is touched, naming the function."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_nearest_cross_pruned_workspace_bytes", "dc_hip_nearest_neighbors_cross_pruned_dev",
         "dc_hip_nearest_cross_pruned_info_dev")
FN = b"dc_hip_nearest_neighbors_cross_pruned_dev"


def test_the_symbols_are_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    assert re.search(r"DC_API\s+size_t\s+" + NAMES[0] + r"\s*\(", text)
    for name in NAMES[1:]:
        assert re.search(r"DC_API\s+int\s+" + name + r"\s*\(", text), name
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_workspace_rule():
    from clustering_amd import capi
    f, plain = capi.lib.dc_hip_nearest_cross_pruned_workspace_bytes, capi.lib.dc_hip_cross_workspace_bytes
    shapes = ((1, 1), (31, 2311), (1037, 33), (200000, 1000000))
    for d in (1, 2, 10, 33, 64):
        for n_q, n_r in shapes:
            assert f(n_q, n_r, d) > 0 and f(n_q, n_r, d) >= plain(n_q, n_r, d), (n_q, n_r, d)
    for d in (65, 100, 401):
        assert f(1000, 1000, d) == 0, d
    for d in (3, 10, 64):
        sizes = [1, 31, 32, 33, 1000, 1001, 4096, 100000, 1000000]
        for fixed in (1, 1000, 50000):
            by_q = [f(n, fixed, d) for n in sizes]
            by_r = [f(fixed, n, d) for n in sizes]
            assert by_q == sorted(by_q) and by_r == sorted(by_r), (d, fixed)
            assert by_q[-1] > by_q[0] and by_r[-1] > by_r[0]
    # the existing pins stay: no variant value of the every-variant query or of the every-variant sweep
    assert capi.lib.dc_hip_cross_workspace_bytes_for(1000, 1000, 10, 6) == 0


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    call = lib.dc_hip_nearest_neighbors_cross_pruned_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    # beyond 64 columns, like DC_VARIANT_MFMA
    assert call(None, 10, None, 10, 65, None, None, 0, 10, None, None, None, None, None, 0, None) == -1
    assert FN in lib.dc_hip_last_error()
    # fe_query without fe_ref
    assert call(None, 10, None, 10, 3, fake, None, 0, 10, None, None, None, None, None, 0, None) == -1
    assert FN in lib.dc_hip_last_error() and b"d_fe_ref" in lib.dc_hip_last_error()
    # frame ids must fit uint32: DC_ERR_TOO_LARGE (-4)
    assert call(None, 10, None, 2 ** 32 - 1, 3, None, None, 0, 10, None, None, None, None, None, 0, None) == -4
    assert FN in lib.dc_hip_last_error()
    assert call(None, 2 ** 32, None, 10, 3, None, None, 0, 10, None, None, None, None, None, 0, None) == -4
    assert FN in lib.dc_hip_last_error()
    # the every-variant sweep keeps refusing the population sweep's variant value
    assert lib.dc_hip_nearest_neighbors_cross_dev(None, 10, None, 10, 3, None, None, 0, 10, None, None, None, None,
                                                  None, 0, 5, None) == -1
    # the info call without a workspace
    assert lib.dc_hip_nearest_cross_pruned_info_dev(None, None, None, None, None) == -1
