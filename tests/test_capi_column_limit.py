"""The column bound of the C ABI: rows of any width up to 2^32 - 65 columns are accepted; wider rows, whose column
count the kernels could not carry, are refused with DC_ERR_TOO_LARGE before anything touches a device.  CPU only: no
call here reaches the GPU (the refusals come first; the accepted calls have no rows)."""
import ctypes as C

import numpy as np
import pytest

DC_OK, DC_ERR_TOO_LARGE = 0, -4
MAX_COLS = 2**32 - 65
TOO_WIDE = [MAX_COLS + 1, 2**32 - 31, 2**32 - 1, 2**32, 2**32 + 401, 2**40]


@pytest.fixture(scope="module")
def lib():
    from clustering_amd import capi
    return capi.lib


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n_cols", TOO_WIDE)
def test_too_wide_rows_are_refused_by_every_entry_point(lib, n_cols):
    n = 2
    c = np.zeros(16, dtype=np.float32)           # (never read: every call below is refused first)
    r = np.array([0.5], dtype=np.float32)
    u = np.zeros(16, dtype=np.uint32)
    f = np.zeros(16, dtype=np.float32)
    w = np.zeros(16, dtype=np.uint64)
    rp = r.ctypes.data_as(C.POINTER(C.c_float))
    calls = {
        "populations_dev": lambda: lib.dc_hip_populations_dev(vp(c), n, n_cols, rp, 1, 0, n, vp(u), None, 0, 1, None),
        "populations_segment_dev": lambda: lib.dc_hip_populations_segment_dev(vp(c), n, n_cols, rp, 1, 0, 2, vp(u),
                                                                            None, 0, 1, None),
        "nearest_neighbors_dev": lambda: lib.dc_hip_nearest_neighbors_dev(vp(c), n, n_cols, vp(f), 0, n, vp(u), vp(f),
                                                                        vp(u), vp(f), None, 0, 1, None),
        "nearest_neighbors_segment_dev": lambda: lib.dc_hip_nearest_neighbors_segment_dev(
            vp(c), n, n_cols, vp(f), 0, 2, vp(u), vp(f), vp(u), vp(f), None, 0, 1, None),
        "neighbors_block_pack_dev": lambda: lib.dc_hip_neighbors_block_pack_dev(vp(u), vp(f), vp(u), vp(f), n, n_cols,
                                                                              0, 2, None, 0, 1, vp(u), None),
        "neighbors_block_unpack_dev": lambda: lib.dc_hip_neighbors_block_unpack_dev(vp(u), n, n_cols, 2, None, 0, 1,
                                                                                  vp(u), vp(f), vp(u), vp(f), None),
        "radius_pairs_dev": lambda: lib.dc_hip_radius_pairs_dev(vp(c), n, n_cols, 0.25, vp(u), None, 0, vp(w), None, 0,
                                                              None),
        "radius_min_edge_dev": lambda: lib.dc_hip_radius_min_edge_dev(vp(c), n, n_cols, 0.25, vp(u), vp(u), vp(w),
                                                                    vp(u), None, 0, None),
        "radius_min_edge_segment_dev": lambda: lib.dc_hip_radius_min_edge_segment_dev(
            vp(c), n, n_cols, 0.25, vp(u), vp(u), 0, 2, vp(w), vp(u), None, 0, None),
        "populations": lambda: lib.dc_hip_populations(vp(c), n, n_cols, vp(r), 1, 0, n, 0, vp(u)),
        "nearest_neighbors": lambda: lib.dc_hip_nearest_neighbors(vp(c), n, n_cols, vp(f), 0, n, 0, vp(u), vp(f),
                                                                  vp(u), vp(f)),
        "session_open": lambda: lib.dc_hip_session_open(vp(c), n, n_cols, None, 0, C.byref(C.c_void_p(0))),
        "density_all": lambda: lib.dc_hip_density_all(vp(c), n, n_cols, vp(r), 1, 0, 0, vp(u), None, None, None, None,
                                                      None),
        "radius_pairs": lambda: lib.dc_hip_radius_pairs(vp(c), n, n_cols, 0.25, 0, None, 0, C.byref(C.c_uint64(0))),
        "radius_forest": lambda: lib.dc_hip_radius_forest(vp(c), n, n_cols, 0.25, vp(u), 0, vp(u),
                                                          C.byref(C.c_size_t(0)), C.byref(C.c_uint32(0))),
    }
    for name, call in calls.items():
        assert call() == DC_ERR_TOO_LARGE, name
        assert b"columns" in lib.dc_hip_last_error(), name


def test_widest_accepted_row(lib):
    """the bound itself is accepted (no rows: nothing to sweep, nothing reaches a device)"""
    r = np.array([0.5], dtype=np.float32)
    rp = r.ctypes.data_as(C.POINTER(C.c_float))
    for n_cols in (401, 10**6, MAX_COLS):
        assert lib.dc_hip_populations_dev(None, 0, n_cols, rp, 1, 0, 0, None, None, 0, 1, None) == DC_OK, n_cols
        assert lib.dc_hip_populations(None, 0, n_cols, r.ctypes.data_as(C.c_void_p), 1, 0, 0, 0, None) == DC_OK
    assert lib.dc_hip_populations_dev(None, 0, MAX_COLS + 1, rp, 1, 0, 0, None, None, 0, 1, None) == DC_ERR_TOO_LARGE
