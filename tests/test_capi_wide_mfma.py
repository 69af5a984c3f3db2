"""CPU: the interface of the matrix-core sweeps for rows of 65..256 columns: the four entry points are declared, listed and
exported by all three builds, the ABI number stays, the workspace query follows its rule, and the refusals come back
before a device is touched, naming the function."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_wide_workspace_bytes", "dc_hip_populations_wide_dev", "dc_hip_nearest_neighbors_wide_dev",
         "dc_hip_wide_info_dev")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5


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
    # no variant value of its own: the table of the Python host is what it was
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_workspace_rule():
    from clustering_amd import capi
    f = capi.lib.dc_hip_wide_workspace_bytes
    for d in (1, 10, 64, 257, 400, 1000):
        for n in (1, 1000, 200000):
            assert f(n, d, 1) == 0, (n, d)
    sizes = [1, 31, 32, 33, 127, 128, 129, 1000, 1001, 4096, 100000, 1000000]
    for d in (65, 100, 128, 256):
        by_n = [f(n, d, 1) for n in sizes]
        assert by_n[0] > 0 and by_n == sorted(by_n) and by_n[-1] > by_n[0], d
        assert f(1000, d, 8) == f(1000, d, 1)
    assert f(1000, 256, 1) > f(1000, 65, 1)
    # the pins of the existing queries stay
    assert capi.lib.dc_hip_workspace_bytes(1000, 70, 1) == 0
    assert capi.lib.dc_hip_cross_workspace_bytes_for(1000, 1000, 10, 6) == 0


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    pop, nn = lib.dc_hip_populations_wide_dev, lib.dc_hip_nearest_neighbors_wide_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    rad = (ctypes.c_float * 1)(0.5)
    for d in (64, 257, 0, 10):
        assert pop(fake, 10, d, rad, 1, 0, 10, fake, fake, 1 << 30, None) == INVALID, d
        assert b"dc_hip_populations_wide_dev" in lib.dc_hip_last_error()
        assert nn(fake, 10, d, fake, 0, 10, fake, fake, fake, fake, fake, 1 << 30, None) == INVALID, d
        assert b"dc_hip_nearest_neighbors_wide_dev" in lib.dc_hip_last_error()
    # a workspace one byte short, and none at all
    need = lib.dc_hip_wide_workspace_bytes(10, 100, 1)
    assert pop(fake, 10, 100, rad, 1, 0, 10, fake, fake, need - 1, None) == WORKSPACE
    assert b"dc_hip_populations_wide_dev" in lib.dc_hip_last_error()
    assert pop(fake, 10, 100, rad, 1, 0, 10, fake, None, 0, None) == WORKSPACE
    assert nn(fake, 10, 100, fake, 0, 10, fake, fake, fake, fake, fake, need - 1, None) == WORKSPACE
    assert b"dc_hip_nearest_neighbors_wide_dev" in lib.dc_hip_last_error()
    # frame ids must fit uint32; row ranges inside the rows
    assert pop(fake, 2 ** 32, 100, rad, 1, 0, 10, fake, fake, 1 << 30, None) == TOO_LARGE
    assert nn(fake, 2 ** 32, 100, fake, 0, 10, fake, fake, fake, fake, fake, 1 << 30, None) == TOO_LARGE
    assert pop(fake, 10, 100, rad, 1, 5, 4, fake, fake, 1 << 30, None) == INVALID
    assert nn(fake, 10, 100, fake, 0, 11, fake, fake, fake, fake, fake, 1 << 30, None) == INVALID
    # null arrays
    assert pop(None, 10, 100, rad, 1, 0, 10, fake, fake, 1 << 30, None) == INVALID
    assert nn(fake, 10, 100, None, 0, 10, fake, fake, fake, fake, fake, 1 << 30, None) == INVALID
    # the info call without a workspace
    assert lib.dc_hip_wide_info_dev(None, None, None, None, None) == INVALID


def test_calls_with_zero_rows_return_ok():
    from clustering_amd import capi
    lib = capi.lib
    rad = (ctypes.c_float * 1)(0.5)
    for d in (65, 256):
        assert lib.dc_hip_populations_wide_dev(None, 0, d, rad, 1, 0, 0, None, None, 0, None) == 0
        assert lib.dc_hip_populations_wide_dev(None, 10, d, rad, 0, 0, 10, None, None, 0, None) == 0   # no radii
        assert lib.dc_hip_nearest_neighbors_wide_dev(None, 0, d, None, 0, 0, None, None, None, None, None, 0, None) == 0
