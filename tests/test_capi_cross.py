"""CPU: the cross-sweep entry points (queries against a reference trajectory) are declared, listed and exported by all
three builds, and their workspace rule holds (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS = ("dc_hip_cross_workspace_bytes", "dc_hip_populations_cross_dev", "dc_hip_nearest_neighbors_cross_dev",
         "dc_hip_free_energies_scaled_dev", "dc_hip_populations_cross", "dc_hip_nearest_neighbors_cross")


def test_cross_symbols_are_declared_and_listed():
    from clustering_amd import capi
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in CROSS:
        assert re.search(r"DC_API\s+[\w\s\*]+?\b" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS, name
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_cross_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in CROSS:
        assert hasattr(lib, name), (libdir, name)


def test_cross_workspace_rule():
    from clustering_amd import capi
    f = capi.lib.dc_hip_cross_workspace_bytes
    for d in (1, 2, 10, 33, 64):
        for n_q, n_r in ((1, 1), (31, 2311), (1037, 33), (200000, 1000000)):
            assert f(n_q, n_r, d) > 0, (n_q, n_r, d)
    assert f(1000, 1000, 64) < f(1000, 2000, 64) and f(1000, 1000, 64) < f(2000, 1000, 64)
    for d in (65, 100, 401, 5000):
        assert f(1000, 1000, d) == 0, d
    # the self sweeps' workspace rule is untouched
    assert capi.lib.dc_hip_workspace_bytes(1000, 70, 1) == 0


def test_cross_calls_refuse_bad_arguments_before_touching_a_device():
    """argument checks come first: no device is needed to be told no"""
    from clustering_amd import capi
    lib = capi.lib
    r = (ctypes.c_float * 1)(0.5)
    # n_cols = 0
    assert lib.dc_hip_populations_cross_dev(None, 10, None, 10, 0, r, 1, 0, 10, None, None, 0, 0, None) == -1
    # row range outside the queries
    assert lib.dc_hip_populations_cross_dev(None, 10, None, 10, 3, r, 1, 0, 11, None, None, 0, 0, None) == -1
    # variants the cross sweeps do not take, and the statistics flag
    for v in (capi.VARIANT_MFMA_PRUNED, capi.VARIANTS["mfma32"], capi.FLAG_STATS_VALID):
        assert lib.dc_hip_populations_cross_dev(None, 10, None, 10, 3, r, 1, 0, 10, None, None, 0, v, None) == -1, v
        assert lib.dc_hip_nearest_neighbors_cross_dev(None, 10, None, 10, 3, None, None, 0, 10, None, None, None, None,
                                                      None, 0, v, None) == -1, v
    # mfma beyond 64 columns
    assert lib.dc_hip_populations_cross_dev(None, 10, None, 10, 65, r, 1, 0, 10, None, None, 0, capi.VARIANT_MFMA,
                                            None) == -1
    # frame ids that do not fit uint32
    assert lib.dc_hip_nearest_neighbors_cross_dev(None, 10, None, 2 ** 32 - 1, 3, None, None, 0, 10, None, None, None,
                                                  None, None, 0, 0, None) == -4
    # max_pop = 0
    assert lib.dc_hip_free_energies_scaled_dev(None, 10, 0, None, None) == -1
