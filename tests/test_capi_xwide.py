"""CPU: the interface of the matrix-core sweeps for rows of 257..1024 columns: the six entry points are declared, listed and
exported by all three builds, the ABI number and the variant table stay, the workspace queries follow their rule (and the
65..256 queries keep refusing these widths), and the refusals come back before a device is touched, naming the function."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_NAMES = ("dc_hip_xwide_workspace_bytes", "dc_hip_cross_xwide_workspace_bytes")
CALL_NAMES = ("dc_hip_populations_xwide_dev", "dc_hip_nearest_neighbors_xwide_dev", "dc_hip_populations_cross_xwide_dev",
              "dc_hip_nearest_neighbors_cross_xwide_dev")
NAMES = SIZE_NAMES + CALL_NAMES
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
BIG = 1 << 40   # a byte count no layout of ten rows reaches


def test_the_symbols_are_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in SIZE_NAMES:
        assert re.search(r"DC_API\s+size_t\s+" + name + r"\s*\(", text), name
    for name in CALL_NAMES:
        assert re.search(r"DC_API\s+int\s+" + name + r"\s*\(", text), name
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib, name), name
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


def test_workspace_rule():
    from clustering_amd import capi
    f, g = capi.lib.dc_hip_xwide_workspace_bytes, capi.lib.dc_hip_cross_xwide_workspace_bytes
    for d in (0, 1, 64, 65, 256, 1025, 4000):
        for n in (1, 1000, 200000):
            assert f(n, d, 1) == 0, (n, d)
            assert g(n, n, d, 1) == 0, (n, d)
    sizes = [1, 31, 32, 33, 127, 128, 129, 1000, 1001, 4096, 100000, 1000000]
    for d in (257, 400, 512, 1024):
        assert f(0, d, 1) == 0 and g(0, 10, d, 1) == 0 and g(10, 0, d, 1) == 0
        by_n = [f(n, d, 1) for n in sizes]
        assert by_n[0] > 0 and by_n == sorted(by_n) and by_n[-1] > by_n[0], d
        assert f(1000, d, 8) == f(1000, d, 1)
        by_q = [g(n, 1000, d, 1) for n in sizes]
        by_r = [g(1000, n, d, 1) for n in sizes]
        assert by_q[0] > 0 and by_q == sorted(by_q) and by_q[-1] > by_q[0], d
        assert by_r[0] > 0 and by_r == sorted(by_r) and by_r[-1] > by_r[0], d
        # both images lie behind the header and its [1024] sums and [1024] means: byte 13 312
        assert f(1, d, 1) > 13312
    assert f(1000, 1024, 1) > f(1000, 257, 1) and g(1000, 1000, 1024, 1) > g(1000, 1000, 257, 1)
    # about 6 KB per row and image at 1024 columns: 193 MFMAs x 32 bytes x 2 images, then the norms and the merge words
    assert 2 * 193 * 32 * 100000 < f(100000, 1024, 1) < 2 * 193 * 32 * 100000 * 1.01
    # the queries of 65..256 columns keep refusing these widths
    assert capi.lib.dc_hip_wide_workspace_bytes(1000, 257, 1) == 0
    assert capi.lib.dc_hip_cross_wide_workspace_bytes(1000, 1000, 257, 1) == 0
    # ... and their layout is what it was: 256 and 257 columns are 49 MFMAs both, so the two byte counts differ by the
    # statistics regions alone (1024 + [256] sums + [256] means = 4096 against 13 312)
    assert capi.lib.dc_hip_wide_workspace_bytes(1000, 256, 1) == f(1000, 257, 1) - (13312 - 4096)


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    pop, nn = lib.dc_hip_populations_xwide_dev, lib.dc_hip_nearest_neighbors_xwide_dev
    xpop, xnn = lib.dc_hip_populations_cross_xwide_dev, lib.dc_hip_nearest_neighbors_cross_xwide_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    rad = (ctypes.c_float * 1)(0.5)

    def refused(status, name, rc):
        assert rc == status, (name, rc)
        assert name.encode() in lib.dc_hip_last_error(), (name, lib.dc_hip_last_error())

    def calls(n, d, lo, hi, ws, ws_bytes, coords=fake, fe=fake):
        """the four entry points over n rows (the cross ones: n queries against n reference rows)"""
        return (("dc_hip_populations_xwide_dev", lambda: pop(coords, n, d, rad, 1, lo, hi, fake, ws, ws_bytes, None)),
                ("dc_hip_nearest_neighbors_xwide_dev", lambda: nn(coords, n, d, fe, lo, hi, fake, fake, fake, fake, ws, ws_bytes, None)),
                ("dc_hip_populations_cross_xwide_dev", lambda: xpop(coords, n, fake, n, d, rad, 1, lo, hi, fake, ws, ws_bytes, None)),
                ("dc_hip_nearest_neighbors_cross_xwide_dev",
                 lambda: xnn(coords, n, fake, n, d, fe, fake, lo, hi, fake, fake, fake, fake, ws, ws_bytes, None)))

    for d in (0, 64, 256, 1025):
        for name, call in calls(10, d, 0, 10, fake, BIG):
            refused(INVALID, name, call())
            assert b"257..1024" in lib.dc_hip_last_error(), lib.dc_hip_last_error()
    # a workspace one byte short, and none at all
    for d in (257, 1024):
        need = {0: lib.dc_hip_xwide_workspace_bytes(10, d, 1), 2: lib.dc_hip_cross_xwide_workspace_bytes(10, 10, d, 1)}
        for k, (name, call) in enumerate(calls(10, d, 0, 10, fake, 0)):
            short = calls(10, d, 0, 10, fake, need[k & 2] - 1)[k][1]
            none = calls(10, d, 0, 10, None, BIG)[k][1]
            refused(WORKSPACE, name, short())
            refused(WORKSPACE, name, none())
    # frame ids must fit uint32 (checked before the row range and the pointers)
    for name, call in calls(2 ** 32, 300, 0, 10, fake, BIG):
        refused(TOO_LARGE, name, call())
    # ranges outside the rows
    for lo, hi in ((5, 4), (0, 11), (11, 11)):
        for name, call in calls(10, 300, lo, hi, fake, BIG):
            refused(INVALID, name, call())
    # null arrays
    for name, call in calls(10, 300, 0, 10, fake, BIG, coords=None):
        refused(INVALID, name, call())
    refused(INVALID, "dc_hip_nearest_neighbors_xwide_dev", nn(fake, 10, 300, None, 0, 10, fake, fake, fake, fake, fake, BIG, None))
    refused(INVALID, "dc_hip_populations_xwide_dev", pop(fake, 10, 300, rad, 1, 0, 10, None, fake, BIG, None))
    refused(INVALID, "dc_hip_populations_cross_xwide_dev", xpop(fake, 10, None, 10, 300, rad, 1, 0, 10, fake, fake, BIG, None))
    # (free energies of the queries without those of the reference)
    refused(INVALID, "dc_hip_nearest_neighbors_cross_xwide_dev",
            xnn(fake, 10, fake, 10, 300, fake, None, 0, 10, fake, fake, fake, fake, fake, BIG, None))
    # the width is checked first: a call that is wrong in every way is refused for its width
    refused(INVALID, "dc_hip_populations_xwide_dev", pop(None, 2 ** 32, 256, rad, 1, 5, 4, None, None, 0, None))
    assert b"257..1024" in lib.dc_hip_last_error()


def test_calls_with_zero_rows_or_zero_radii_return_ok():
    from clustering_amd import capi
    lib = capi.lib
    rad = (ctypes.c_float * 1)(0.5)
    for d in (257, 1024):
        assert lib.dc_hip_populations_xwide_dev(None, 0, d, rad, 1, 0, 0, None, None, 0, None) == 0
        assert lib.dc_hip_populations_xwide_dev(None, 10, d, rad, 0, 0, 10, None, None, 0, None) == 0   # no radii
        assert lib.dc_hip_nearest_neighbors_xwide_dev(None, 0, d, None, 0, 0, None, None, None, None, None, 0, None) == 0
        assert lib.dc_hip_populations_cross_xwide_dev(None, 0, None, 10, d, rad, 1, 0, 0, None, None, 0, None) == 0
        assert lib.dc_hip_populations_cross_xwide_dev(None, 10, None, 10, d, rad, 0, 0, 10, None, None, 0, None) == 0
        assert lib.dc_hip_nearest_neighbors_cross_xwide_dev(None, 0, None, 10, d, None, None, 0, 0, None, None, None, None,
                                                            None, 0, None) == 0
