"""CPU: the interface of the pruned self sweeps at 257..1024 columns: the four entry points are declared, listed and
exported by all three builds, the ABI number and the variants stay, the workspace query follows its rule (and the query of
65..256 columns stays 0 at 257), and every refusal comes back before a device is touched, naming the function."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_xwide_pruned_workspace_bytes", "dc_hip_populations_xwide_pruned_dev",
         "dc_hip_nearest_neighbors_xwide_pruned_dev", "dc_hip_xwide_pruned_order_dev")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
BIG = 1 << 34


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
    for fn in ("calculate_populations_xwide_pruned", "nearest_neighbors_xwide_pruned", "xwide_pruned_info", "xwide_pruned_order"):
        assert callable(getattr(density, fn)), fn
    assert "xwide_pruned" in density._SIZES, "a cached workspace of a kind of its own"


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_workspace_rule():
    from clustering_amd import capi
    f, g = capi.lib.dc_hip_xwide_pruned_workspace_bytes, capi.lib.dc_hip_xwide_workspace_bytes
    for d in (0, 1, 64, 65, 256, 1025):
        for n in (1, 1000, 200000):
            assert f(n, d, 1) == 0, (n, d)
    sizes = [1, 31, 32, 33, 127, 128, 129, 1000, 1001, 4096, 8320, 100000, 1000000]
    for d in (257, 400, 512, 1024):
        assert f(0, d, 1) == 0
        by_n = [f(n, d, 1) for n in sizes]
        assert by_n[0] > 0 and by_n == sorted(by_n) and by_n[-1] > by_n[0], d
        for n, b in zip(sizes, by_n):
            assert b > g(n, d, 1) > 0, "the unpruned layout is its head; the order lies behind it"
        assert f(1000, d, 8) == f(1000, d, 1) == f(1000, d, 11)
    by_d = [f(1000, d, 1) for d in (257, 400, 512, 1024)]
    assert by_d == sorted(by_d) and by_d[-1] > by_d[0]
    # the head of these widths: the images start at byte 13 312, not at 4 096 -- one row of 257 columns takes more than
    # the whole 256-column layout of one row would at that offset
    assert f(1, 257, 1) - capi.lib.dc_hip_wide_pruned_workspace_bytes(1, 256, 1) >= 13312 - 4096
    # the queries of the other families stay what they were
    w = capi.lib.dc_hip_wide_pruned_workspace_bytes
    assert w(1000, 257, 1) == 0 and w(1000, 1024, 1) == 0 and w(1000, 256, 1) > 0
    assert g(1000, 256, 1) == 0


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    pop, nn, order = (lib.dc_hip_populations_xwide_pruned_dev, lib.dc_hip_nearest_neighbors_xwide_pruned_dev,
                      lib.dc_hip_xwide_pruned_order_dev)
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    rad = (ctypes.c_float * 1)(0.5)
    err = lib.dc_hip_last_error
    for d in (0, 10, 64, 65, 256, 1025):
        assert pop(fake, 10, d, rad, 1, 0, 0, fake, fake, BIG, None) == INVALID, d
        assert NAMES[1].encode() in err() and b"257..1024" in err()
        assert nn(fake, 10, d, fake, 0, 0, fake, fake, fake, fake, fake, BIG, None) == INVALID, d
        assert NAMES[2].encode() in err() and b"257..1024" in err()
        assert order(fake, 10, d, fake, None) == INVALID, d
        assert NAMES[3].encode() in err() and b"257..1024" in err()
    # ... and the entry points of 65..256 columns still refuse these widths
    assert lib.dc_hip_populations_wide_pruned_dev(fake, 10, 257, rad, 1, 0, 0, fake, fake, BIG, None) == INVALID
    assert lib.dc_hip_nearest_neighbors_wide_pruned_dev(fake, 10, 257, fake, 0, 0, fake, fake, fake, fake, fake, BIG, None) == INVALID
    assert lib.dc_hip_wide_pruned_order_dev(fake, 10, 257, fake, None) == INVALID
    # a segment that is none of the n_segments
    for seg, nseg in ((1, 1), (2, 2), (7, 3), (2 ** 40, 5)):
        assert pop(fake, 10, 300, rad, 1, seg, nseg, fake, fake, BIG, None) == INVALID, (seg, nseg)
        assert NAMES[1].encode() in err()
        assert nn(fake, 10, 300, fake, seg, nseg, fake, fake, fake, fake, fake, BIG, None) == INVALID, (seg, nseg)
        assert NAMES[2].encode() in err()
    for d in (257, 1024):
        need = lib.dc_hip_xwide_pruned_workspace_bytes(10, d, 1)
        # a workspace one byte short, and none at all
        assert pop(fake, 10, d, rad, 1, 0, 0, fake, fake, need - 1, None) == WORKSPACE
        assert NAMES[1].encode() in err()
        assert pop(fake, 10, d, rad, 1, 0, 0, fake, None, 0, None) == WORKSPACE
        assert pop(fake, 10, d, rad, 1, 1, 2, fake, None, BIG, None) == WORKSPACE
        assert nn(fake, 10, d, fake, 0, 0, fake, fake, fake, fake, fake, need - 1, None) == WORKSPACE
        assert NAMES[2].encode() in err()
        assert nn(fake, 10, d, fake, 0, 0, fake, fake, fake, fake, None, 0, None) == WORKSPACE
        # the byte count of the unpruned sweeps of these widths is too small for the order
        plain = lib.dc_hip_xwide_workspace_bytes(1000, d, 1)
        assert 0 < plain < lib.dc_hip_xwide_pruned_workspace_bytes(1000, d, 1)
        assert pop(fake, 1000, d, rad, 1, 0, 0, fake, fake, plain, None) == WORKSPACE
        assert nn(fake, 1000, d, fake, 0, 0, fake, fake, fake, fake, fake, plain, None) == WORKSPACE
    # frame ids must fit uint32, and the elements the index arithmetic
    assert pop(fake, 2 ** 32, 300, rad, 1, 0, 0, fake, fake, BIG, None) == TOO_LARGE
    assert NAMES[1].encode() in err()
    assert pop(fake, 2 ** 31, 1024, rad, 1, 0, 0, fake, fake, BIG, None) == TOO_LARGE
    assert nn(fake, 2 ** 32, 300, fake, 0, 0, fake, fake, fake, fake, fake, BIG, None) == TOO_LARGE
    assert NAMES[2].encode() in err()
    assert order(fake, 2 ** 32, 300, fake, None) == TOO_LARGE
    # null arrays
    assert pop(None, 10, 300, rad, 1, 0, 0, fake, fake, BIG, None) == INVALID
    assert pop(fake, 10, 300, None, 1, 0, 0, fake, fake, BIG, None) == INVALID
    assert pop(fake, 10, 300, rad, 1, 0, 0, None, fake, BIG, None) == INVALID
    for k in (0, 3, 6, 7, 8, 9):   # coords, fe, and each of the four outputs
        args = [fake, 10, 300, fake, 0, 0, fake, fake, fake, fake, fake, BIG, None]
        args[k] = None
        assert nn(*args) == INVALID, k
        assert NAMES[2].encode() in err() and b"null" in err()
    # no workspace holds no order
    assert order(None, 10, 300, fake, None) == INVALID and order(fake, 0, 300, fake, None) == INVALID
    assert order(fake, 10, 300, None, None) == INVALID


def test_calls_with_nothing_to_do_return_ok():
    from clustering_amd import capi
    lib = capi.lib
    rad = (ctypes.c_float * 1)(0.5)
    for d in (257, 1024):
        for seg, nseg in ((0, 0), (5, 0), (2, 3)):   # n_segments == 0: the whole sweep, `segment` is not read
            assert lib.dc_hip_populations_xwide_pruned_dev(None, 0, d, rad, 1, seg, nseg, None, None, 0, None) == 0
            assert lib.dc_hip_nearest_neighbors_xwide_pruned_dev(None, 0, d, None, seg, nseg, None, None, None, None, None, 0, None) == 0
        assert lib.dc_hip_populations_xwide_pruned_dev(None, 10, d, rad, 0, 0, 0, None, None, 0, None) == 0   # no radii
