"""CPU: the interface of the pruned population sweep against a reference (DC_VARIANT_CROSS_PRUNED): the workspace
query dc_hip_cross_workspace_bytes_for is declared, listed and exported by all three builds and follows its rule, and
every entry point that does not take the variant says so in its argument checks -- no device is needed to be told no."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dc_hip_cross_workspace_bytes_for"
CROSS_PRUNED = 5


def test_the_symbol_is_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    assert re.search(r"DC_API\s+size_t\s+" + NAME + r"\s*\(", text)
    assert re.search(r"DC_VARIANT_CROSS_PRUNED\s*=\s*5\b", text)
    assert NAME in capi.SYMBOLS
    assert capi.VARIANTS["cross_pruned"] == CROSS_PRUNED == capi.VARIANT_CROSS_PRUNED
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbol(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    assert hasattr(ctypes.CDLL(path), NAME), libdir


def test_workspace_rule_of_every_variant():
    from clustering_amd import capi
    f, plain = capi.lib.dc_hip_cross_workspace_bytes_for, capi.lib.dc_hip_cross_workspace_bytes
    shapes = ((1, 1), (31, 2311), (1037, 33), (200000, 1000000))
    for d in (1, 2, 10, 33, 64):
        for n_q, n_r in shapes:
            for v in (0, 1, 2):
                assert f(n_q, n_r, d, v) == plain(n_q, n_r, d) > 0, (n_q, n_r, d, v)
            assert f(n_q, n_r, d, CROSS_PRUNED) > plain(n_q, n_r, d), (n_q, n_r, d)
            for v in (3, 4, 6, 0x100, 0x105):
                assert f(n_q, n_r, d, v) == 0, (n_q, n_r, d, v)
    for d in (65, 100, 401):
        for v in (0, 1, 2, 3, 4, CROSS_PRUNED):
            assert f(1000, 1000, d, v) == 0, (d, v)
    # monotone in either row count
    for d in (3, 10, 64):
        sizes = [1, 31, 32, 33, 1000, 1001, 4096, 100000, 1000000]
        for fixed in (1, 1000, 50000):
            by_q = [f(n, fixed, d, CROSS_PRUNED) for n in sizes]
            by_r = [f(fixed, n, d, CROSS_PRUNED) for n in sizes]
            assert by_q == sorted(by_q) and by_r == sorted(by_r), (d, fixed)
            assert by_q[-1] > by_q[0] and by_r[-1] > by_r[0]


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    r = (ctypes.c_float * 1)(0.5)
    v = CROSS_PRUNED
    # beyond 64 columns, like DC_VARIANT_MFMA there
    assert lib.dc_hip_populations_cross_dev(None, 10, None, 10, 65, r, 1, 0, 10, None, None, 0, v, None) == -1
    # no flags on a cross call
    assert lib.dc_hip_populations_cross_dev(None, 10, None, 10, 3, r, 1, 0, 10, None, None, 0,
                                            v | capi.FLAG_STATS_VALID, None) == -1
    # the neighbour sweep against a reference has no pruned form
    assert lib.dc_hip_nearest_neighbors_cross_dev(None, 10, None, 10, 3, None, None, 0, 10, None, None, None, None,
                                                  None, 0, v, None) == -1
    # the self sweeps: an unknown value would be treated like auto, so the refusal is explicit
    for flags in (0, capi.FLAG_STATS_VALID):
        assert lib.dc_hip_populations_dev(None, 10, 3, r, 1, 0, 10, None, None, 0, v | flags, None) == -1
        assert lib.dc_hip_populations_segment_dev(None, 10, 3, r, 1, 0, 2, None, None, 0, v | flags, None) == -1
        assert lib.dc_hip_nearest_neighbors_dev(None, 10, 3, None, 0, 10, None, None, None, None, None, 0, v | flags,
                                                None) == -1
        assert lib.dc_hip_nearest_neighbors_segment_dev(None, 10, 3, None, 0, 2, None, None, None, None, None, 0,
                                                        v | flags, None) == -1
    assert lib.dc_hip_neighbors_block_pack_dev(None, None, None, None, 10, 3, 0, 2, None, 0, v, None, None) == -1
    assert lib.dc_hip_neighbors_block_unpack_dev(None, 10, 3, 2, None, 0, v, None, None, None, None, None) == -1
    assert b"CROSS_PRUNED" in lib.dc_hip_last_error()
