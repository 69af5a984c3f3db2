"""CPU: the C ABI of the fp32-input matrix-core sweeps for rows of 1..32 columns (dc_hip_fp32_workspace_bytes,
dc_hip_fp32_plan, dc_hip_populations_fp32_dev, dc_hip_nearest_neighbors_fp32_dev): the symbols in header, library and
binding, every refusal with its status code and message -- each issued before a device is touched, so the calls here pass
fake pointers that are never dereferenced -- and the planner over the whole grid of shapes."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, TOO_LARGE, WORKSPACE = 0, -1, -4, -5
FAKE = ctypes.c_void_p(64)
BIG = 1 << 40
NAMES = ("dc_hip_fp32_workspace_bytes", "dc_hip_fp32_plan", "dc_hip_populations_fp32_dev", "dc_hip_nearest_neighbors_fp32_dev")
RADII = np.array([0.5, 0.25], dtype=np.float32)


@pytest.fixture(scope="module")
def lib():
    from clustering_amd import capi
    return capi.lib


def _radii(null=False):
    return None if null else RADII.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def pop(lib, n=10, d=5, radii=False, n_radii=2, a=0, b=None, coords=FAKE, pops=FAKE, ws=FAKE, wb=BIG):
    return lib.dc_hip_populations_fp32_dev(coords, n, d, _radii(radii), n_radii, a, n if b is None else b, pops, ws, wb, None)


def nn(lib, n=10, d=5, a=0, b=None, null=None, ws=FAKE, wb=BIG):
    p = lambda name: None if null == name else FAKE   # noqa: E731
    return lib.dc_hip_nearest_neighbors_fp32_dev(p("coords"), n, d, p("fe"), a, n if b is None else b, p("nn_idx"), p("nn_d2"),
                                                 p("hd_idx"), p("hd_d2"), ws, wb, None)


def refused(lib, rc, status, *texts):
    msg = lib.dc_hip_last_error().decode()
    assert rc == status, (rc, msg)
    assert all(t in msg for t in texts), msg


def test_symbols_in_header_library_and_binding(lib):
    from clustering_amd import capi
    header = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in NAMES:
        assert name in capi.SYMBOLS
        assert re.search(r"DC_API\s+\w+\s+" + name + r"\(", header), name
        assert getattr(lib, name) is not None
    assert capi.lib.dc_hip_abi_version() == 5
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}


def test_workspace_bytes(lib):
    f = lib.dc_hip_fp32_workspace_bytes
    assert f(1000, 0, 1) == 0 and f(1000, 33, 1) == 0 and f(0, 5, 1) == 0
    assert f(1000, 1, 1) > 0 and f(1000, 32, 1) > 0
    for d in (1, 5, 10, 30, 32):
        assert f(1000, d, 3) == lib.dc_hip_workspace_bytes(1000, d, 3)
        assert f(2000, d, 1) >= f(1000, d, 1)


@pytest.mark.parametrize("d", (0, 33, 64, 100))
def test_column_counts_outside_1_to_32_are_refused(lib, d):
    refused(lib, pop(lib, d=d), INVALID, "dc_hip_populations_fp32_dev", "1..32")
    refused(lib, nn(lib, d=d), INVALID, "dc_hip_nearest_neighbors_fp32_dev", "1..32")
    out = (ctypes.c_uint32 * 8)()
    refused(lib, lib.dc_hip_fp32_plan(100, d, 1, out), INVALID, "dc_hip_fp32_plan", "1..32")


def test_no_radii_are_refused(lib):
    refused(lib, pop(lib, n_radii=0), INVALID, "n_radii")
    out = (ctypes.c_uint32 * 8)()
    refused(lib, lib.dc_hip_fp32_plan(100, 5, 0, out), INVALID, "n_radii")
    refused(lib, lib.dc_hip_fp32_plan(0, 5, 1, out), INVALID, "n_rows")
    refused(lib, lib.dc_hip_fp32_plan(100, 5, 65536, out), TOO_LARGE, "65535")
    refused(lib, pop(lib, n_radii=65536), TOO_LARGE, "65535")
    assert lib.dc_hip_fp32_plan(100, 5, 65535, out) == OK and out[3] == (8 | (8192 << 16))


def test_null_pointers_are_refused(lib):
    refused(lib, pop(lib, coords=None), INVALID, "null pointer")
    refused(lib, pop(lib, radii=True), INVALID, "null pointer")
    refused(lib, pop(lib, pops=None), INVALID, "null pointer")
    for name in ("coords", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2"):
        refused(lib, nn(lib, null=name), INVALID, "null pointer")
    refused(lib, lib.dc_hip_fp32_plan(100, 5, 1, None), INVALID, "null pointer")


def test_a_missing_or_short_workspace_is_refused(lib):
    need = lib.dc_hip_fp32_workspace_bytes(10, 5, 2)
    refused(lib, pop(lib, ws=None, wb=0), WORKSPACE, str(need), "got 0")
    refused(lib, pop(lib, wb=need - 1), WORKSPACE, str(need), str(need - 1))
    refused(lib, pop(lib, ws=None, wb=BIG), WORKSPACE, str(need))
    refused(lib, nn(lib, ws=None, wb=0), WORKSPACE, str(need), "got 0")
    refused(lib, nn(lib, wb=need - 1), WORKSPACE, str(need), str(need - 1))


def test_row_ranges_out_of_order_or_beyond_the_rows_are_refused(lib):
    refused(lib, pop(lib, a=3, b=2), INVALID, "row range [3, 2)")
    refused(lib, pop(lib, a=0, b=11), INVALID, "row range [0, 11)")
    refused(lib, nn(lib, a=3, b=2), INVALID, "row range [3, 2)")
    refused(lib, nn(lib, a=0, b=11), INVALID, "row range [0, 11)")


def test_rows_beyond_the_index_type_are_refused(lib):
    refused(lib, pop(lib, n=2 ** 32), TOO_LARGE, "uint32")
    refused(lib, nn(lib, n=2 ** 32 - 1), TOO_LARGE, "uint32")
    out = (ctypes.c_uint32 * 8)()
    refused(lib, lib.dc_hip_fp32_plan(2 ** 32, 5, 1, out), TOO_LARGE, "uint32")
    assert lib.dc_hip_fp32_workspace_bytes(2 ** 32, 5, 1) == 0


def test_no_rows_is_ok_without_a_device(lib):
    assert pop(lib, n=0, ws=None, wb=0) == OK
    assert nn(lib, n=0, ws=None, wb=0) == OK



@pytest.mark.parametrize("n_cols", range(1, 33))
def test_the_plan_over_the_grid_of_shapes(n_cols):
    from clustering_amd import density
    exact = (n_cols + 1) // 2
    for n_radii in (1, 2, 3, 8, 9, 17):
        for n_rows in (1, 32, 33, 257, 20_000, 1_000_000):
            p = density.fp32_sweep_plan(n_rows, n_cols, n_radii)
            # the documented pad step: the even step counts below 16 run the next odd instance
            assert p["k_steps"] == (exact + 1 if (exact % 2 == 0 and exact < 16) else exact), p
            if n_cols in (5, 10, 30):
                assert p["k_steps"] == exact, "exact at the widths of the five configurations"
            assert p["lane_floats"] % 4 == 0 and p["lane_floats"] >= p["k_steps"] and p["lane_floats"] < p["k_steps"] + 4
            assert p["sweeps"] == -(-n_radii // 8) and p["radii_per_sweep"] == min(n_radii, 8)
            assert p["tq_pop"] in (4, 8) and p["tq_nn"] in (2, 4)
            assert 0 < p["lds_pop"] <= 160 * 1024 and 0 < p["lds_nn"] <= 160 * 1024
            assert p["image_bytes_per_tile"] == 256 * p["lane_floats"]
            assert p["image_bytes_per_tile"] <= p["image_region_bytes_per_tile"]
            assert p["image_region_bytes_per_tile"] == 1024 * -(-(3 * n_cols + 2) // 16), "the region of make_layout"
            tiles = -(-n_rows // 32)
            assert 1 <= p["chunks_pop"] <= 16 and 1 <= p["chunks_nn"] <= 16
            assert p["chunks_pop"] == 1 or tiles // p["chunks_pop"] >= 512


def test_the_chunk_switch_reaches_the_plan():
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); from clustering_amd import density; "
            "p = density.fp32_sweep_plan(1500, 30, 3); print(p['chunks_pop'], p['chunks_nn'])" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DC_MFMA32_CHUNKS="3"), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["3", "3"], r.stdout + r.stderr
