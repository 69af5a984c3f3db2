"""CPU: the interface of the pruned cross sweeps at 257..1024 columns: the four entry points are declared, listed and exported
by all three builds, the ABI number and the variants stay, the workspace query follows its rule and the two families of
widths stay apart in both directions, every refusal comes back before a device is touched, naming the function -- and the
byte counts of the 65..256 family are the parent's: folding the bodies behind one form moved none."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_cross_xwide_pruned_workspace_bytes", "dc_hip_populations_cross_xwide_pruned_dev",
         "dc_hip_nearest_neighbors_cross_xwide_pruned_dev", "dc_hip_cross_xwide_pruned_order_dev")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
BIG = 1 << 34
# dc_hip_cross_wide_pruned_workspace_bytes(n_query, n_ref, n_cols, n_radii) of the library before this change
PINNED = {(300, 1500, 65, 1): 1332480, (1500, 1500, 100, 1): 3195904, (700, 2100, 128, 4): 3892736, (1, 300, 200, 1): 880384,
          (1100, 8320, 256, 8): 24800512, (129, 300, 255, 1): 1444096}


def test_the_symbols_are_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    assert re.search(r"DC_API\s+size_t\s+" + NAMES[0] + r"\s*\(", text)
    for name in NAMES[1:]:
        assert re.search(r"DC_API\s+int\s+" + name + r"\s*\(", text), name
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib, name), name
    assert len(set(capi.SYMBOLS)) == len(capi.SYMBOLS)
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}
    for fn in ("calculate_populations_against_xwide_pruned", "nearest_reference_xwide_pruned", "xwide_against_pruned_info",
               "xwide_against_pruned_order", "assign_frames_xwide_pruned"):
        assert callable(getattr(density, fn)), fn
    assert "xwide_against_pruned" in density._SIZES, "a cached workspace of a kind of its own"


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_the_byte_counts_of_65_to_256_columns_are_the_parents():
    from clustering_amd import capi
    for args, want in PINNED.items():
        assert capi.lib.dc_hip_cross_wide_pruned_workspace_bytes(*args) == want, args


def test_workspace_rule():
    from clustering_amd import capi
    f, g = capi.lib.dc_hip_cross_xwide_pruned_workspace_bytes, capi.lib.dc_hip_cross_xwide_workspace_bytes
    w = capi.lib.dc_hip_cross_wide_pruned_workspace_bytes
    for d in (0, 1, 64, 65, 256, 1025):
        for n_q, n_r in ((1, 1), (1000, 5000), (200000, 200000)):
            assert f(n_q, n_r, d, 1) == 0, (n_q, n_r, d)
    sizes = [1, 31, 32, 33, 127, 128, 129, 1000, 1001, 4096, 8320, 100000, 1000000]
    for d in (257, 400, 512, 1024):
        assert f(0, 1000, d, 1) == 0 and f(1000, 0, d, 1) == 0 and f(0, 0, d, 1) == 0, "an empty side"
        by_q = [f(n, 1000, d, 1) for n in sizes]
        by_r = [f(1000, n, d, 1) for n in sizes]
        for by in (by_q, by_r):
            assert by[0] > 0 and by == sorted(by) and by[-1] > by[0], d
        for n in sizes:
            assert f(n, 1000, d, 1) > g(n, 1000, d, 1) > 0 and f(1000, n, d, 1) > g(1000, n, d, 1) > 0, \
                "the unpruned layout is its head; the orders lie behind it"
        assert f(1000, 3000, d, 8) == f(1000, 3000, d, 1) == f(1000, 3000, d, 11)
    by_d = [f(1000, 3000, d, 1) for d in (257, 400, 512, 1024)]
    assert by_d == sorted(by_d) and by_d[-1] > by_d[0]
    # the two families stay apart, in both directions: 256 | 257
    assert w(1000, 3000, 257, 1) == 0 and w(1000, 3000, 1024, 1) == 0 and w(1000, 3000, 256, 1) > 0
    assert f(1000, 3000, 256, 1) == 0 and f(1000, 3000, 257, 1) > 0
    # the head of these widths: the images start at byte 13 312, not at 4 096
    assert f(1, 1, 257, 1) - w(1, 1, 256, 1) >= 13312 - 4096
    assert g(1000, 3000, 256, 1) == 0


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    pop, nn, order = (lib.dc_hip_populations_cross_xwide_pruned_dev, lib.dc_hip_nearest_neighbors_cross_xwide_pruned_dev,
                      lib.dc_hip_cross_xwide_pruned_order_dev)
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    rad = (ctypes.c_float * 1)(0.5)
    err = lib.dc_hip_last_error
    nn_args = lambda n_q, n_r, d, ws, ws_bytes: [fake, n_q, fake, n_r, d, fake, fake, 0, n_q, fake, fake, fake, fake, ws, ws_bytes, None]
    for d in (0, 10, 64, 65, 256, 1025):
        assert pop(fake, 10, fake, 20, d, rad, 1, 0, 10, fake, fake, BIG, None) == INVALID, d
        assert NAMES[1].encode() in err() and b"257..1024" in err()
        assert nn(*nn_args(10, 20, d, fake, BIG)) == INVALID, d
        assert NAMES[2].encode() in err() and b"257..1024" in err()
        assert order(fake, 10, 20, d, fake, fake, None) == INVALID, d
        assert NAMES[3].encode() in err() and b"257..1024" in err()
    # ... and the entry points of 65..256 columns still refuse these widths, naming themselves
    assert lib.dc_hip_populations_cross_wide_pruned_dev(fake, 10, fake, 20, 257, rad, 1, 0, 10, fake, fake, BIG, None) == INVALID
    assert b"dc_hip_populations_cross_wide_pruned_dev" in err() and b"65..256" in err()
    assert lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev(*nn_args(10, 20, 257, fake, BIG)) == INVALID
    assert b"dc_hip_nearest_neighbors_cross_wide_pruned_dev" in err() and b"65..256" in err()
    assert lib.dc_hip_cross_wide_pruned_order_dev(fake, 10, 20, 257, fake, fake, None) == INVALID
    assert b"dc_hip_cross_wide_pruned_order_dev" in err() and b"65..256" in err()
    # a row range outside the queries
    for lo, hi in ((5, 4), (0, 11), (11, 11)):
        assert pop(fake, 10, fake, 20, 300, rad, 1, lo, hi, fake, fake, BIG, None) == INVALID, (lo, hi)
        assert NAMES[1].encode() in err() and b"row range" in err()
        args = nn_args(10, 20, 300, fake, BIG)
        args[7], args[8] = lo, hi
        assert nn(*args) == INVALID, (lo, hi)
        assert NAMES[2].encode() in err() and b"row range" in err()
    for d in (257, 1024):
        need = lib.dc_hip_cross_xwide_pruned_workspace_bytes(10, 20, d, 1)
        # a workspace one byte short, and none at all
        assert pop(fake, 10, fake, 20, d, rad, 1, 0, 10, fake, fake, need - 1, None) == WORKSPACE
        assert NAMES[1].encode() in err()
        assert pop(fake, 10, fake, 20, d, rad, 1, 0, 10, fake, None, 0, None) == WORKSPACE
        assert pop(fake, 10, fake, 20, d, rad, 1, 0, 10, fake, None, BIG, None) == WORKSPACE
        assert nn(*nn_args(10, 20, d, fake, need - 1)) == WORKSPACE
        assert NAMES[2].encode() in err()
        assert nn(*nn_args(10, 20, d, None, 0)) == WORKSPACE
        # the byte counts of the unpruned cross sweeps and of the pruned self sweeps of these widths are too small
        # (3 000 rows against 3 000: the self sweep of as many rows holds one gathered set, one order, one set of boxes)
        plain = lib.dc_hip_cross_xwide_workspace_bytes(3000, 3000, d, 1)
        self_pruned = lib.dc_hip_xwide_pruned_workspace_bytes(3000, d, 1)
        full = lib.dc_hip_cross_xwide_pruned_workspace_bytes(3000, 3000, d, 1)
        assert 0 < plain < self_pruned < full
        for short in (plain, self_pruned):
            assert pop(fake, 3000, fake, 3000, d, rad, 1, 0, 3000, fake, fake, short, None) == WORKSPACE
            assert NAMES[1].encode() in err()
            assert nn(*nn_args(3000, 3000, d, fake, short)) == WORKSPACE
            assert NAMES[2].encode() in err()
    # frame ids must fit uint32, and the elements the index arithmetic
    assert pop(fake, 2 ** 32, fake, 20, 300, rad, 1, 0, 10, fake, fake, BIG, None) == TOO_LARGE
    assert NAMES[1].encode() in err()
    assert pop(fake, 10, fake, 2 ** 32 - 1, 300, rad, 1, 0, 10, fake, fake, BIG, None) == TOO_LARGE
    assert pop(fake, 10, fake, 2 ** 31, 1024, rad, 1, 0, 10, fake, fake, BIG, None) == TOO_LARGE
    assert nn(*nn_args(2 ** 32, 20, 300, fake, BIG)) == TOO_LARGE
    assert NAMES[2].encode() in err()
    assert order(fake, 2 ** 32, 20, 300, fake, fake, None) == TOO_LARGE
    assert NAMES[3].encode() in err()
    # null arrays
    for k in (0, 2, 5, 9):   # queries, reference, radii, populations
        args = [fake, 10, fake, 20, 300, rad, 1, 0, 10, fake, fake, BIG, None]
        args[k] = None
        assert pop(*args) == INVALID, k
        assert NAMES[1].encode() in err() and b"null" in err()
    for k in (0, 2, 6, 9, 10, 11, 12):   # queries, reference, fe_ref beside fe_query, and each of the four outputs
        args = nn_args(10, 20, 300, fake, BIG)
        args[k] = None
        assert nn(*args) == INVALID, k
        assert NAMES[2].encode() in err() and b"null" in err()
    # no workspace holds no order
    assert order(None, 10, 20, 300, fake, fake, None) == INVALID and NAMES[3].encode() in err()
    assert order(fake, 0, 20, 300, fake, fake, None) == INVALID and order(fake, 10, 0, 300, fake, fake, None) == INVALID
    assert order(fake, 10, 20, 300, None, fake, None) == INVALID and order(fake, 10, 20, 300, fake, None, None) == INVALID


def test_calls_with_nothing_to_do_return_ok():
    from clustering_amd import capi
    lib = capi.lib
    rad = (ctypes.c_float * 1)(0.5)
    for d in (257, 1024):
        assert lib.dc_hip_populations_cross_xwide_pruned_dev(None, 0, None, 0, d, rad, 1, 0, 0, None, None, 0, None) == 0
        assert lib.dc_hip_populations_cross_xwide_pruned_dev(None, 10, None, 20, d, rad, 0, 0, 10, None, None, 0, None) == 0   # no radii
        assert lib.dc_hip_nearest_neighbors_cross_xwide_pruned_dev(None, 0, None, 0, d, None, None, 0, 0, None, None, None, None,
                                                                   None, 0, None) == 0
