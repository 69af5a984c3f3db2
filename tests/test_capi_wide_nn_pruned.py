"""CPU: the interface of the pruned wide neighbour sweep: the entry point is declared, listed and exported by all three
builds, the ABI number and the variants stay, the workspace query of the pruned wide sweeps gives what it gave before,
and every refusal comes back before a device is touched, naming the function."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dc_hip_nearest_neighbors_wide_pruned_dev"
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
# dc_hip_wide_pruned_workspace_bytes(n_rows, n_cols, 1) of the commit before this entry point existed
WORKSPACE_PINS = {(1, 65): 115968, (300, 100): 617216, (2100, 100): 3654400, (8320, 80): 11825920,
                  (100000, 256): 423970048, (200000, 100): 338608640}


def test_the_symbol_is_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    assert re.search(r"DC_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in capi.SYMBOLS and hasattr(capi.lib, NAME)
    assert capi.lib.dc_hip_nearest_neighbors_wide_pruned_dev.argtypes == capi.lib.dc_hip_nearest_neighbors_wide_dev.argtypes
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}
    for fn in ("nearest_neighbors_wide_pruned", "wide_pruned_info", "wide_pruned_order"):
        assert callable(getattr(density, fn)), fn


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbol(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    assert hasattr(ctypes.CDLL(path), NAME), libdir


def test_the_workspace_query_gives_what_it_gave():
    from clustering_amd import capi
    f = capi.lib.dc_hip_wide_pruned_workspace_bytes
    for (n, d), want in WORKSPACE_PINS.items():
        assert f(n, d, 1) == want == f(n, d, 8), (n, d)
    assert f(1000, 64, 1) == 0 and f(1000, 257, 1) == 0 and f(0, 100, 1) == 0


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    nn = lib.dc_hip_nearest_neighbors_wide_pruned_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    name = NAME.encode()
    big = 1 << 30
    for d in (64, 257, 0, 10):
        assert nn(fake, 10, d, fake, 0, 0, fake, fake, fake, fake, fake, big, None) == INVALID, d
        assert name in lib.dc_hip_last_error()
    # a segment that is none of the n_segments
    for seg, nseg in ((1, 1), (2, 2), (7, 3), (2 ** 40, 5)):
        assert nn(fake, 10, 100, fake, seg, nseg, fake, fake, fake, fake, fake, big, None) == INVALID, (seg, nseg)
        assert name in lib.dc_hip_last_error()
    # a workspace one byte short, and none at all
    need = lib.dc_hip_wide_pruned_workspace_bytes(10, 100, 1)
    assert nn(fake, 10, 100, fake, 0, 0, fake, fake, fake, fake, fake, need - 1, None) == WORKSPACE
    assert name in lib.dc_hip_last_error()
    assert nn(fake, 10, 100, fake, 0, 0, fake, fake, fake, fake, None, 0, None) == WORKSPACE
    assert nn(fake, 10, 100, fake, 1, 2, fake, fake, fake, fake, None, big, None) == WORKSPACE
    # the unpruned sweeps' workspace is too small for the order
    assert nn(fake, 1000, 100, fake, 0, 0, fake, fake, fake, fake, fake, lib.dc_hip_wide_workspace_bytes(1000, 100, 1), None) == WORKSPACE
    # frame ids must fit uint32, and the elements the index arithmetic
    assert nn(fake, 2 ** 32, 100, fake, 0, 0, fake, fake, fake, fake, fake, big, None) == TOO_LARGE
    assert name in lib.dc_hip_last_error()
    assert nn(fake, 2 ** 31, 256, fake, 0, 0, fake, fake, fake, fake, fake, big, None) == TOO_LARGE
    # null arrays, each of the six
    for k in (0, 3, 6, 7, 8, 9):
        args = [fake, 10, 100, fake, 0, 0, fake, fake, fake, fake, fake, big, None]
        args[k] = None
        assert nn(*args) == INVALID, k
        assert name in lib.dc_hip_last_error()


def test_calls_with_nothing_to_do_return_ok():
    from clustering_amd import capi
    nn = capi.lib.dc_hip_nearest_neighbors_wide_pruned_dev
    for d in (65, 256):
        assert nn(None, 0, d, None, 0, 0, None, None, None, None, None, 0, None) == 0
        assert nn(None, 0, d, None, 2, 3, None, None, None, None, None, 0, None) == 0
