"""CPU: the interface of the pruned wide cross population sweep: the three entry points are declared, listed and exported
by all three builds, the ABI number stays, the workspace query follows its rule, and every refusal comes back before a
device is touched, naming the function."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_cross_wide_pruned_workspace_bytes", "dc_hip_populations_cross_wide_pruned_dev",
         "dc_hip_cross_wide_pruned_order_dev")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5


def test_the_symbols_are_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    assert re.search(r"DC_API\s+size_t\s+" + NAMES[0] + r"\s*\(", text)
    for name in NAMES[1:]:
        assert re.search(r"DC_API\s+int\s+" + name + r"\s*\(", text), name
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}
    for fn in ("calculate_populations_against_wide_pruned", "wide_against_pruned_info", "wide_against_pruned_order",
               "assign_frames_wide_pruned"):
        assert callable(getattr(density, fn)), fn


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_workspace_rule():
    from clustering_amd import capi
    f, g = capi.lib.dc_hip_cross_wide_pruned_workspace_bytes, capi.lib.dc_hip_cross_wide_workspace_bytes
    for d in (0, 1, 10, 64, 257, 400, 1000):
        for n_q, n_r in ((1, 1), (1000, 200000), (200000, 1000)):
            assert f(n_q, n_r, d, 1) == 0, (n_q, n_r, d)
    sizes = [1, 31, 32, 33, 127, 128, 129, 1000, 1001, 4096, 8320, 100000, 1000000]
    for d in (65, 100, 128, 256):
        assert f(0, 100, d, 1) == 0 and f(100, 0, d, 1) == 0 and f(0, 0, d, 1) == 0, "an empty side needs no workspace"
        for fixed in (1, 300, 20000):
            by_q = [f(n, fixed, d, 1) for n in sizes]
            by_r = [f(fixed, n, d, 1) for n in sizes]
            for by in (by_q, by_r):
                assert by[0] > 0 and by == sorted(by) and by[-1] > by[0], (d, fixed)
            for n, bq, br in zip(sizes, by_q, by_r):
                assert bq >= g(n, fixed, d, 1) and br >= g(fixed, n, d, 1), "never below the unpruned cross sweeps' workspace"
        assert f(1000, 700, d, 8) == f(1000, 700, d, 1) == f(1000, 700, d, 11)
    assert f(1000, 1000, 256, 1) > f(1000, 1000, 65, 1)
    # the pins of the existing queries stay
    assert g(1000, 1000, 64, 1) == 0 and g(1000, 1000, 100, 1) > 0 and g(0, 1000, 100, 1) == 0
    assert capi.lib.dc_hip_wide_pruned_workspace_bytes(1000, 64, 1) == 0


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    pop, order = lib.dc_hip_populations_cross_wide_pruned_dev, lib.dc_hip_cross_wide_pruned_order_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    rad = (ctypes.c_float * 1)(0.5)
    name = b"dc_hip_populations_cross_wide_pruned_dev"
    for d in (64, 257, 0, 10):
        assert pop(fake, 10, fake, 20, d, rad, 1, 0, 10, fake, fake, 1 << 30, None) == INVALID, d
        assert name in lib.dc_hip_last_error()
        assert order(fake, 10, 20, d, fake, fake, None) == INVALID, d
        assert b"dc_hip_cross_wide_pruned_order_dev" in lib.dc_hip_last_error()
    # a range that is none of the queries'
    for lo, hi in ((5, 4), (0, 11), (11, 11), (2 ** 40, 2 ** 40 + 1)):
        assert pop(fake, 10, fake, 20, 100, rad, 1, lo, hi, fake, fake, 1 << 30, None) == INVALID, (lo, hi)
        assert name in lib.dc_hip_last_error()
    # a workspace one byte short, and none at all
    need = lib.dc_hip_cross_wide_pruned_workspace_bytes(10, 20, 100, 1)
    assert pop(fake, 10, fake, 20, 100, rad, 1, 0, 10, fake, fake, need - 1, None) == WORKSPACE
    assert name in lib.dc_hip_last_error()
    assert pop(fake, 10, fake, 20, 100, rad, 1, 0, 10, fake, None, 0, None) == WORKSPACE
    assert pop(fake, 10, fake, 20, 100, rad, 1, 3, 3, fake, None, 1 << 30, None) == WORKSPACE, "the workspace check comes before the range is looked at"
    # the unpruned cross sweeps' workspace is too small for the orders
    assert pop(fake, 1000, fake, 700, 100, rad, 1, 0, 1000, fake, fake, lib.dc_hip_cross_wide_workspace_bytes(1000, 700, 100, 1),
               None) == WORKSPACE
    # frame ids must fit uint32, and the elements the index arithmetic
    assert pop(fake, 2 ** 32, fake, 20, 100, rad, 1, 0, 1, fake, fake, 1 << 30, None) == TOO_LARGE
    assert pop(fake, 10, fake, 2 ** 32 - 1, 100, rad, 1, 0, 1, fake, fake, 1 << 30, None) == TOO_LARGE
    assert pop(fake, 2 ** 31, fake, 20, 256, rad, 1, 0, 1, fake, fake, 1 << 30, None) == TOO_LARGE
    assert pop(fake, 10, fake, 2 ** 31, 256, rad, 1, 0, 1, fake, fake, 1 << 30, None) == TOO_LARGE
    assert order(fake, 2 ** 32, 20, 100, fake, fake, None) == TOO_LARGE
    assert order(fake, 10, 2 ** 32 - 1, 100, fake, fake, None) == TOO_LARGE
    # null arrays
    assert pop(None, 10, fake, 20, 100, rad, 1, 0, 10, fake, fake, 1 << 30, None) == INVALID
    assert pop(fake, 10, None, 20, 100, rad, 1, 0, 10, fake, fake, 1 << 30, None) == INVALID
    assert pop(fake, 10, fake, 20, 100, None, 1, 0, 10, fake, fake, 1 << 30, None) == INVALID
    assert pop(fake, 10, fake, 20, 100, rad, 1, 0, 10, None, fake, 1 << 30, None) == INVALID
    # no workspace, no query range and no reference hold no order
    assert order(None, 10, 20, 100, fake, fake, None) == INVALID
    assert order(fake, 0, 20, 100, fake, fake, None) == INVALID and order(fake, 10, 0, 100, fake, fake, None) == INVALID
    assert order(fake, 10, 20, 100, None, fake, None) == INVALID and order(fake, 10, 20, 100, fake, None, None) == INVALID


def test_calls_with_nothing_to_write_return_ok():
    from clustering_amd import capi
    pop = capi.lib.dc_hip_populations_cross_wide_pruned_dev
    rad = (ctypes.c_float * 1)(0.5)
    for d in (65, 256):
        assert pop(None, 0, None, 0, d, rad, 1, 0, 0, None, None, 0, None) == 0
        assert pop(None, 0, None, 40, d, rad, 1, 0, 0, None, None, 0, None) == 0      # no queries
        assert pop(None, 10, None, 20, d, rad, 0, 0, 10, None, None, 0, None) == 0    # no radii
