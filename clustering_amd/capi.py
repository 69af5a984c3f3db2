"""ctypes binding of the C ABI in include/dc_density.h (clustering_amd/lib/libdcdensity.so).

There is deliberately no fallback: if the HIP library is missing or cannot be loaded,
importing this module raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C clustering_amd/csrc``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DC_LIB_PATH: another build of the SAME library (measurement variants under clustering_amd/lib/variants/) instead of
# copying it over the product.  DC_CANON_ORDER=avx: the build with the summation order of a reference compiled
# with -DCPU_ACCELERATION=AVX (`make -C clustering_amd/csrc CANON=avx` -> clustering_amd/lib_avx/; dc_hip_canon_order());
# DC_CANON_ORDER=fma: that of a -DNATIVE_COMPILATION build on an AVX2 + FMA host (CANON=fma -> clustering_amd/lib_fma/)
CANON_ORDER = os.environ.get("DC_CANON_ORDER", "sse2")
_CANON_DIRS = {"sse2": "lib", "avx": "lib_avx", "fma": "lib_fma"}
if CANON_ORDER not in _CANON_DIRS:
    raise ImportError(f"DC_CANON_ORDER={CANON_ORDER!r}: expected 'sse2' (the reference's default build), 'avx' or 'fma'")
LIB_PATH = os.environ.get("DC_LIB_PATH") or os.path.join(_HERE, _CANON_DIRS[CANON_ORDER], "libdcdensity.so")

DC_OK, DC_ERR_INVALID_ARGUMENT, DC_ERR_HIP = 0, -1, -3
ABI_VERSION = 5               # include/dc_density.h: DC_HIP_ABI_VERSION this binding was written against
FLAG_STATS_VALID = 0x100      # DC_FLAG_STATS_VALID
VARIANT_AUTO, VARIANT_DIRECT, VARIANT_MFMA, VARIANT_MFMA_PRUNED = 0, 1, 2, 3
VARIANT_CROSS_PRUNED = 5      # dc_hip_populations_cross_dev only
VARIANTS = {"auto": VARIANT_AUTO, "direct": VARIANT_DIRECT, "mfma": VARIANT_MFMA,
            "pruned": VARIANT_MFMA_PRUNED, "mfma32": 4, "cross_pruned": VARIANT_CROSS_PRUNED}

# every symbol include/dc_density.h declares (tests/test_capi_symbols.py checks the header against this)
SYMBOLS = (
    "dc_hip_last_error", "dc_hip_abi_version", "dc_hip_build_digest", "dc_hip_canon_order", "dc_hip_device_count", "dc_hip_workspace_bytes",
    "dc_hip_populations_dev", "dc_hip_free_energies_dev", "dc_hip_nearest_neighbors_dev",
    "dc_hip_sigma2_dev", "dc_hip_workspace_counters_dev", "dc_hip_workspace_mfma_counters_dev", "dc_hip_workspace_layout_status_dev", "dc_hip_sweep_timing", "dc_hip_last_sweep_ms", "dc_hip_workspace_components_dev", "dc_hip_populations", "dc_hip_nearest_neighbors", "dc_hip_density_all",
    "dc_hip_radius_pairs_dev", "dc_hip_radius_pairs", "dc_hip_radius_min_edge_dev", "dc_hip_radius_forest",
    "dc_hip_populations_segment_dev", "dc_hip_nearest_neighbors_segment_dev",
    "dc_hip_neighbors_pack_dev", "dc_hip_neighbors_unpack_dev", "dc_hip_neighbors_block_rows",
    "dc_hip_neighbors_block_pack_dev", "dc_hip_neighbors_block_unpack_dev", "dc_hip_radius_min_edge_segment_dev",
    "dc_hip_session_open", "dc_hip_session_close", "dc_hip_session_devices", "dc_hip_session_uses_rccl",
    "dc_hip_session_merge_mode", "dc_hip_session_merge_note",
    "dc_hip_session_counters", "dc_hip_session_populations", "dc_hip_session_free_energies",
    "dc_hip_session_set_free_energies", "dc_hip_session_nearest_neighbors", "dc_hip_session_radius_pairs",
    "dc_hip_session_radius_forest",
    "dc_hip_cross_workspace_bytes", "dc_hip_populations_cross_dev", "dc_hip_nearest_neighbors_cross_dev",
    "dc_hip_free_energies_scaled_dev", "dc_hip_populations_cross", "dc_hip_nearest_neighbors_cross",
    "dc_hip_cross_workspace_bytes_for",
    "dc_hip_nearest_cross_pruned_workspace_bytes", "dc_hip_nearest_neighbors_cross_pruned_dev",
    "dc_hip_nearest_cross_pruned_info_dev",
    "dc_hip_wide_workspace_bytes", "dc_hip_populations_wide_dev", "dc_hip_nearest_neighbors_wide_dev", "dc_hip_wide_info_dev",
    "dc_hip_cross_wide_workspace_bytes", "dc_hip_populations_cross_wide_dev", "dc_hip_nearest_neighbors_cross_wide_dev",
    "dc_hip_xwide_workspace_bytes", "dc_hip_populations_xwide_dev", "dc_hip_nearest_neighbors_xwide_dev",
    "dc_hip_cross_xwide_workspace_bytes", "dc_hip_populations_cross_xwide_dev", "dc_hip_nearest_neighbors_cross_xwide_dev",
    "dc_hip_radius_pairs_wide_dev", "dc_hip_radius_min_edge_wide_dev", "dc_hip_radius_forest_wide",
    "dc_hip_wide_pruned_workspace_bytes", "dc_hip_populations_wide_pruned_dev", "dc_hip_wide_pruned_order_dev",
    "dc_hip_radius_pairs_wide_pruned_dev", "dc_hip_radius_min_edge_wide_pruned_dev", "dc_hip_radius_forest_wide_pruned",
    "dc_hip_nearest_neighbors_wide_pruned_dev",
    "dc_hip_xwide_pruned_workspace_bytes", "dc_hip_populations_xwide_pruned_dev", "dc_hip_nearest_neighbors_xwide_pruned_dev",
    "dc_hip_xwide_pruned_order_dev",
    "dc_hip_cross_wide_pruned_workspace_bytes", "dc_hip_populations_cross_wide_pruned_dev", "dc_hip_cross_wide_pruned_order_dev",
    "dc_hip_nearest_neighbors_cross_wide_pruned_dev",
    "dc_hip_cross_xwide_pruned_workspace_bytes", "dc_hip_populations_cross_xwide_pruned_dev", "dc_hip_cross_xwide_pruned_order_dev",
    "dc_hip_nearest_neighbors_cross_xwide_pruned_dev",
    "dc_hip_neighbors_block_rows_wide", "dc_hip_neighbors_block_pack_wide_dev", "dc_hip_neighbors_block_unpack_wide_dev",
    "dc_hip_wide_layout_status_dev", "dc_hip_session_open_flags", "dc_hip_session_wide",
    "dc_hip_reference_wide_workspace_bytes", "dc_hip_reference_wide_open_dev", "dc_hip_reference_wide_close",
    "dc_hip_reference_wide_set_free_energies_dev", "dc_hip_reference_wide_stage_dev", "dc_hip_reference_wide_populations_dev",
    "dc_hip_reference_wide_nearest_dev", "dc_hip_reference_wide_info_dev", "dc_hip_reference_wide_order_dev",
    "dc_hip_reference_workspace_bytes", "dc_hip_reference_open_dev", "dc_hip_reference_close",
    "dc_hip_reference_set_free_energies_dev", "dc_hip_reference_stage_dev", "dc_hip_reference_populations_dev",
    "dc_hip_reference_nearest_dev", "dc_hip_reference_info_dev", "dc_hip_reference_order_dev",
    "dc_hip_assign_workspace_bytes", "dc_hip_assign_open_dev", "dc_hip_assign_open_wide_dev", "dc_hip_assign_close",
    "dc_hip_assign_batch_dev",
    "dc_hip_assigner_open", "dc_hip_assigner_reference", "dc_hip_assigner_path", "dc_hip_assigner_assign", "dc_hip_assigner_close",
    "dc_hip_reference_xwide_workspace_bytes", "dc_hip_reference_xwide_open_dev", "dc_hip_reference_xwide_close",
    "dc_hip_reference_xwide_set_free_energies_dev", "dc_hip_reference_xwide_stage_dev", "dc_hip_reference_xwide_populations_dev",
    "dc_hip_reference_xwide_nearest_dev", "dc_hip_reference_xwide_info_dev", "dc_hip_reference_xwide_order_dev",
    "dc_hip_assign_open_xwide_dev", "dc_hip_assigner_open_flags",
    "dc_hip_radius_pairs_xwide_dev", "dc_hip_radius_min_edge_xwide_dev", "dc_hip_radius_forest_xwide",
    "dc_hip_radius_pairs_xwide_pruned_dev", "dc_hip_radius_min_edge_xwide_pruned_dev", "dc_hip_radius_forest_xwide_pruned",
    "dc_hip_neighbors_block_rows_xwide", "dc_hip_neighbors_block_pack_xwide_dev", "dc_hip_neighbors_block_unpack_xwide_dev",
    "dc_hip_xwide_layout_status_dev",
    "dc_hip_fp32_workspace_bytes", "dc_hip_fp32_plan", "dc_hip_populations_fp32_dev", "dc_hip_nearest_neighbors_fp32_dev",
)
SESSION_WIDE_SWEEPS = 0x1     # DC_SESSION_WIDE_SWEEPS (dc_hip_session_open_flags)
ASSIGNER_XWIDE_REFERENCE = 0x1   # DC_ASSIGNER_XWIDE_REFERENCE (dc_hip_assigner_open_flags)


class DensityLibraryError(RuntimeError):
    """status: the C ABI's return code (0 where the error did not come from a call); detail: dc_hip_last_error()"""
    status = 0
    detail = ""


def _load():
    if not os.path.exists(LIB_PATH):
        raise DensityLibraryError(
            f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build()). "
            "clustering_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    lib.dc_hip_last_error.restype = C.c_char_p
    lib.dc_hip_last_error.argtypes = []
    lib.dc_hip_abi_version.restype = i32
    lib.dc_hip_abi_version.argtypes = []
    if lib.dc_hip_abi_version() != ABI_VERSION:
        raise DensityLibraryError(
            f"{LIB_PATH} has ABI version {lib.dc_hip_abi_version()}, this binding needs {ABI_VERSION}: rebuild "
            "the library (python -c 'import __graft_entry__ as g; g.build()')")
    lib.dc_hip_build_digest.restype = C.c_char_p
    lib.dc_hip_build_digest.argtypes = []
    lib.dc_hip_canon_order.restype = C.c_char_p
    lib.dc_hip_canon_order.argtypes = []
    if "DC_LIB_PATH" not in os.environ and lib.dc_hip_canon_order().decode() != CANON_ORDER:
        raise DensityLibraryError(f"{LIB_PATH} reproduces the {lib.dc_hip_canon_order().decode()!r} summation order, "
                                  f"DC_CANON_ORDER asks for {CANON_ORDER!r}: rebuild it")
    lib.dc_hip_device_count.restype = i32
    lib.dc_hip_workspace_bytes.restype = sz
    lib.dc_hip_workspace_bytes.argtypes = [sz, sz, sz]
    lib.dc_hip_populations_dev.restype = i32
    lib.dc_hip_populations_dev.argtypes = [vp, sz, sz, C.POINTER(C.c_float), sz, sz, sz, vp, vp, sz,
                                           i32, vp]
    lib.dc_hip_free_energies_dev.restype = i32
    lib.dc_hip_free_energies_dev.argtypes = [vp, sz, vp, C.POINTER(C.c_uint32), vp]
    lib.dc_hip_nearest_neighbors_dev.restype = i32
    lib.dc_hip_nearest_neighbors_dev.argtypes = [vp, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, sz,
                                                 i32, vp]
    lib.dc_hip_sigma2_dev.restype = i32
    lib.dc_hip_sigma2_dev.argtypes = [vp, sz, C.POINTER(C.c_double), vp]
    lib.dc_hip_workspace_counters_dev.restype = i32
    lib.dc_hip_workspace_counters_dev.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    lib.dc_hip_workspace_components_dev.restype = i32
    lib.dc_hip_workspace_components_dev.argtypes = [vp, sz, sz, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                                    C.POINTER(C.c_float), C.POINTER(C.c_float), vp]
    lib.dc_hip_sweep_timing.restype = i32
    lib.dc_hip_sweep_timing.argtypes = [i32]
    lib.dc_hip_last_sweep_ms.restype = i32
    lib.dc_hip_last_sweep_ms.argtypes = [i32, C.POINTER(C.c_float)]
    lib.dc_hip_populations.restype = i32
    lib.dc_hip_populations.argtypes = [vp, sz, sz, vp, sz, sz, sz, i32, vp]
    lib.dc_hip_nearest_neighbors.restype = i32
    lib.dc_hip_nearest_neighbors.argtypes = [vp, sz, sz, vp, sz, sz, i32, vp, vp, vp, vp]
    lib.dc_hip_populations_segment_dev.restype = i32
    lib.dc_hip_populations_segment_dev.argtypes = [vp, sz, sz, C.POINTER(C.c_float), sz, sz, sz, vp, vp, sz,
                                                   i32, vp]
    lib.dc_hip_nearest_neighbors_segment_dev.restype = i32
    lib.dc_hip_nearest_neighbors_segment_dev.argtypes = [vp, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, sz,
                                                         i32, vp]
    lib.dc_hip_radius_pairs_dev.restype = i32
    lib.dc_hip_radius_pairs_dev.argtypes = [vp, sz, sz, C.c_float, vp, vp, sz, vp, vp, sz, vp]
    lib.dc_hip_radius_pairs.restype = i32
    lib.dc_hip_radius_pairs.argtypes = [vp, sz, sz, C.c_float, i32, vp, sz, C.POINTER(C.c_uint64)]
    lib.dc_hip_neighbors_pack_dev.restype = i32
    lib.dc_hip_neighbors_pack_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp]
    lib.dc_hip_neighbors_unpack_dev.restype = i32
    lib.dc_hip_neighbors_unpack_dev.argtypes = [vp, sz, vp, vp, vp, vp, vp]
    lib.dc_hip_neighbors_block_rows.restype = sz
    lib.dc_hip_neighbors_block_rows.argtypes = [sz, sz, sz]
    lib.dc_hip_neighbors_block_pack_dev.restype = i32
    lib.dc_hip_neighbors_block_pack_dev.argtypes = [vp, vp, vp, vp, sz, sz, sz, sz, vp, sz, i32, vp, vp]
    lib.dc_hip_neighbors_block_unpack_dev.restype = i32
    lib.dc_hip_neighbors_block_unpack_dev.argtypes = [vp, sz, sz, sz, vp, sz, i32, vp, vp, vp, vp, vp]
    lib.dc_hip_radius_min_edge_dev.restype = i32
    lib.dc_hip_radius_min_edge_dev.argtypes = [vp, sz, sz, C.c_float, vp, vp, vp, vp, vp, sz, vp]
    lib.dc_hip_radius_min_edge_segment_dev.restype = i32
    lib.dc_hip_radius_min_edge_segment_dev.argtypes = [vp, sz, sz, C.c_float, vp, vp, sz, sz, vp, vp, vp, sz, vp]
    lib.dc_hip_radius_forest.restype = i32
    lib.dc_hip_radius_forest.argtypes = [vp, sz, sz, C.c_float, vp, i32, vp, C.POINTER(sz),
                                         C.POINTER(C.c_uint32)]
    lib.dc_hip_density_all.restype = i32
    lib.dc_hip_density_all.argtypes = [vp, sz, sz, vp, sz, sz, i32, vp, vp, vp, vp, vp, vp]
    lib.dc_hip_session_open.restype = i32
    lib.dc_hip_session_open.argtypes = [vp, sz, sz, C.POINTER(C.c_int), i32, C.POINTER(vp)]
    lib.dc_hip_session_close.restype = None
    lib.dc_hip_session_close.argtypes = [vp]
    lib.dc_hip_session_devices.restype = i32
    lib.dc_hip_session_devices.argtypes = [vp]
    lib.dc_hip_session_uses_rccl.restype = i32
    lib.dc_hip_session_uses_rccl.argtypes = [vp]
    lib.dc_hip_session_merge_mode.restype = i32
    lib.dc_hip_session_merge_mode.argtypes = [vp]
    lib.dc_hip_workspace_mfma_counters_dev.restype = i32
    lib.dc_hip_workspace_mfma_counters_dev.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    lib.dc_hip_workspace_layout_status_dev.restype = i32
    lib.dc_hip_workspace_layout_status_dev.argtypes = [vp, C.POINTER(C.c_int), vp]
    lib.dc_hip_session_merge_note.restype = C.c_char_p
    lib.dc_hip_session_merge_note.argtypes = [vp]
    lib.dc_hip_session_counters.restype = i32
    lib.dc_hip_session_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.dc_hip_session_populations.restype = i32
    lib.dc_hip_session_populations.argtypes = [vp, vp, sz, vp]
    lib.dc_hip_session_free_energies.restype = i32
    lib.dc_hip_session_free_energies.argtypes = [vp, sz, vp, C.POINTER(C.c_uint32)]
    lib.dc_hip_session_set_free_energies.restype = i32
    lib.dc_hip_session_set_free_energies.argtypes = [vp, vp]
    lib.dc_hip_session_nearest_neighbors.restype = i32
    lib.dc_hip_session_nearest_neighbors.argtypes = [vp, vp, vp, vp, vp, C.POINTER(C.c_double)]
    lib.dc_hip_session_radius_pairs.restype = i32
    lib.dc_hip_session_radius_pairs.argtypes = [vp, C.c_float, vp, sz, C.POINTER(C.c_uint64)]
    lib.dc_hip_session_radius_forest.restype = i32
    lib.dc_hip_session_radius_forest.argtypes = [vp, C.c_float, vp, vp, C.POINTER(sz), C.POINTER(C.c_uint32)]
    lib.dc_hip_cross_workspace_bytes.restype = sz
    lib.dc_hip_cross_workspace_bytes.argtypes = [sz, sz, sz]
    lib.dc_hip_cross_workspace_bytes_for.restype = sz
    lib.dc_hip_cross_workspace_bytes_for.argtypes = [sz, sz, sz, i32]
    lib.dc_hip_populations_cross_dev.restype = i32
    lib.dc_hip_populations_cross_dev.argtypes = [vp, sz, vp, sz, sz, C.POINTER(C.c_float), sz, sz, sz, vp, vp, sz,
                                                 i32, vp]
    lib.dc_hip_nearest_neighbors_cross_dev.restype = i32
    lib.dc_hip_nearest_neighbors_cross_dev.argtypes = [vp, sz, vp, sz, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz,
                                                       i32, vp]
    lib.dc_hip_nearest_cross_pruned_workspace_bytes.restype = sz
    lib.dc_hip_nearest_cross_pruned_workspace_bytes.argtypes = [sz, sz, sz]
    lib.dc_hip_nearest_neighbors_cross_pruned_dev.restype = i32
    lib.dc_hip_nearest_neighbors_cross_pruned_dev.argtypes = [vp, sz, vp, sz, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp]
    lib.dc_hip_nearest_cross_pruned_info_dev.restype = i32
    lib.dc_hip_nearest_cross_pruned_info_dev.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                                         C.POINTER(C.c_uint32), vp]
    lib.dc_hip_wide_workspace_bytes.restype = sz
    lib.dc_hip_wide_workspace_bytes.argtypes = [sz, sz, sz]
    lib.dc_hip_populations_wide_dev.restype = i32
    lib.dc_hip_populations_wide_dev.argtypes = [vp, sz, sz, C.POINTER(C.c_float), sz, sz, sz, vp, vp, sz, vp]
    lib.dc_hip_nearest_neighbors_wide_dev.restype = i32
    lib.dc_hip_nearest_neighbors_wide_dev.argtypes = [vp, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp]
    # the fp32-input MFMA sweeps for 1..32 columns: the argument lists of the wide sweeps, and their host-side planner
    for fp32, wide in (("dc_hip_fp32_workspace_bytes", "dc_hip_wide_workspace_bytes"),
                       ("dc_hip_populations_fp32_dev", "dc_hip_populations_wide_dev"),
                       ("dc_hip_nearest_neighbors_fp32_dev", "dc_hip_nearest_neighbors_wide_dev")):
        getattr(lib, fp32).restype = getattr(lib, wide).restype
        getattr(lib, fp32).argtypes = getattr(lib, wide).argtypes
    lib.dc_hip_fp32_plan.restype = i32
    lib.dc_hip_fp32_plan.argtypes = [sz, sz, sz, C.POINTER(C.c_uint32)]
    lib.dc_hip_wide_info_dev.restype = i32
    lib.dc_hip_wide_info_dev.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    lib.dc_hip_cross_wide_workspace_bytes.restype = sz
    lib.dc_hip_cross_wide_workspace_bytes.argtypes = [sz, sz, sz, sz]
    lib.dc_hip_populations_cross_wide_dev.restype = i32
    lib.dc_hip_populations_cross_wide_dev.argtypes = [vp, sz, vp, sz, sz, C.POINTER(C.c_float), sz, sz, sz, vp, vp, sz, vp]
    lib.dc_hip_nearest_neighbors_cross_wide_dev.restype = i32
    lib.dc_hip_nearest_neighbors_cross_wide_dev.argtypes = [vp, sz, vp, sz, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp]
    for xwide, wide in (("dc_hip_xwide_workspace_bytes", "dc_hip_wide_workspace_bytes"),
                        ("dc_hip_populations_xwide_dev", "dc_hip_populations_wide_dev"),
                        ("dc_hip_nearest_neighbors_xwide_dev", "dc_hip_nearest_neighbors_wide_dev"),
                        ("dc_hip_cross_xwide_workspace_bytes", "dc_hip_cross_wide_workspace_bytes"),
                        ("dc_hip_populations_cross_xwide_dev", "dc_hip_populations_cross_wide_dev"),
                        ("dc_hip_nearest_neighbors_cross_xwide_dev", "dc_hip_nearest_neighbors_cross_wide_dev")):
        getattr(lib, xwide).restype = getattr(lib, wide).restype     # (257..1024 columns: the lists of their namesakes)
        getattr(lib, xwide).argtypes = getattr(lib, wide).argtypes
    lib.dc_hip_radius_pairs_wide_dev.restype = i32
    lib.dc_hip_radius_pairs_wide_dev.argtypes = [vp, sz, sz, C.c_float, vp, vp, sz, vp, vp, sz, vp]
    lib.dc_hip_radius_min_edge_wide_dev.restype = i32
    lib.dc_hip_radius_min_edge_wide_dev.argtypes = [vp, sz, sz, C.c_float, vp, vp, sz, sz, vp, vp, vp, sz, vp]
    lib.dc_hip_radius_forest_wide.restype = i32
    lib.dc_hip_radius_forest_wide.argtypes = [vp, sz, sz, C.c_float, vp, i32, vp, C.POINTER(sz), C.POINTER(C.c_uint32)]
    lib.dc_hip_wide_pruned_workspace_bytes.restype = sz
    lib.dc_hip_wide_pruned_workspace_bytes.argtypes = [sz, sz, sz]
    lib.dc_hip_populations_wide_pruned_dev.restype = i32
    lib.dc_hip_populations_wide_pruned_dev.argtypes = [vp, sz, sz, C.POINTER(C.c_float), sz, sz, sz, vp, vp, sz, vp]
    lib.dc_hip_wide_pruned_order_dev.restype = i32
    lib.dc_hip_wide_pruned_order_dev.argtypes = [vp, sz, sz, vp, vp]
    lib.dc_hip_radius_pairs_wide_pruned_dev.restype = i32
    lib.dc_hip_radius_pairs_wide_pruned_dev.argtypes = lib.dc_hip_radius_pairs_wide_dev.argtypes
    lib.dc_hip_radius_min_edge_wide_pruned_dev.restype = i32
    lib.dc_hip_radius_min_edge_wide_pruned_dev.argtypes = lib.dc_hip_radius_min_edge_wide_dev.argtypes
    lib.dc_hip_radius_forest_wide_pruned.restype = i32
    lib.dc_hip_radius_forest_wide_pruned.argtypes = lib.dc_hip_radius_forest_wide.argtypes
    lib.dc_hip_nearest_neighbors_wide_pruned_dev.restype = i32
    lib.dc_hip_nearest_neighbors_wide_pruned_dev.argtypes = lib.dc_hip_nearest_neighbors_wide_dev.argtypes
    for xwide, wide in (("dc_hip_xwide_pruned_workspace_bytes", "dc_hip_wide_pruned_workspace_bytes"),
                        ("dc_hip_populations_xwide_pruned_dev", "dc_hip_populations_wide_pruned_dev"),
                        ("dc_hip_nearest_neighbors_xwide_pruned_dev", "dc_hip_nearest_neighbors_wide_pruned_dev"),
                        ("dc_hip_xwide_pruned_order_dev", "dc_hip_wide_pruned_order_dev")):
        getattr(lib, xwide).restype = getattr(lib, wide).restype     # (257..1024 columns: the lists of their namesakes)
        getattr(lib, xwide).argtypes = getattr(lib, wide).argtypes
    lib.dc_hip_cross_wide_pruned_workspace_bytes.restype = sz
    lib.dc_hip_cross_wide_pruned_workspace_bytes.argtypes = [sz, sz, sz, sz]
    lib.dc_hip_populations_cross_wide_pruned_dev.restype = i32
    lib.dc_hip_populations_cross_wide_pruned_dev.argtypes = lib.dc_hip_populations_cross_wide_dev.argtypes
    lib.dc_hip_cross_wide_pruned_order_dev.restype = i32
    lib.dc_hip_cross_wide_pruned_order_dev.argtypes = [vp, sz, sz, sz, vp, vp, vp]
    lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev.restype = i32
    lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev.argtypes = lib.dc_hip_nearest_neighbors_cross_wide_dev.argtypes
    for xwide, wide in (("dc_hip_cross_xwide_pruned_workspace_bytes", "dc_hip_cross_wide_pruned_workspace_bytes"),
                        ("dc_hip_populations_cross_xwide_pruned_dev", "dc_hip_populations_cross_wide_pruned_dev"),
                        ("dc_hip_nearest_neighbors_cross_xwide_pruned_dev", "dc_hip_nearest_neighbors_cross_wide_pruned_dev"),
                        ("dc_hip_cross_xwide_pruned_order_dev", "dc_hip_cross_wide_pruned_order_dev")):
        getattr(lib, xwide).restype = getattr(lib, wide).restype     # (257..1024 columns: the lists of their namesakes)
        getattr(lib, xwide).argtypes = getattr(lib, wide).argtypes
    lib.dc_hip_neighbors_block_rows_wide.restype = sz
    lib.dc_hip_neighbors_block_rows_wide.argtypes = [sz, sz, sz]
    lib.dc_hip_neighbors_block_pack_wide_dev.restype = i32
    lib.dc_hip_neighbors_block_pack_wide_dev.argtypes = [vp, vp, vp, vp, sz, sz, sz, sz, vp, sz, vp, vp]
    lib.dc_hip_neighbors_block_unpack_wide_dev.restype = i32
    lib.dc_hip_neighbors_block_unpack_wide_dev.argtypes = [vp, sz, sz, sz, vp, sz, vp, vp, vp, vp, vp]
    lib.dc_hip_wide_layout_status_dev.restype = i32
    lib.dc_hip_wide_layout_status_dev.argtypes = [vp, C.POINTER(C.c_int), vp]
    for xwide, wide in (("dc_hip_radius_pairs_xwide_dev", "dc_hip_radius_pairs_wide_dev"),
                        ("dc_hip_radius_min_edge_xwide_dev", "dc_hip_radius_min_edge_wide_dev"),
                        ("dc_hip_radius_forest_xwide", "dc_hip_radius_forest_wide"),
                        ("dc_hip_radius_pairs_xwide_pruned_dev", "dc_hip_radius_pairs_wide_pruned_dev"),
                        ("dc_hip_radius_min_edge_xwide_pruned_dev", "dc_hip_radius_min_edge_wide_pruned_dev"),
                        ("dc_hip_radius_forest_xwide_pruned", "dc_hip_radius_forest_wide_pruned"),
                        ("dc_hip_neighbors_block_rows_xwide", "dc_hip_neighbors_block_rows_wide"),
                        ("dc_hip_neighbors_block_pack_xwide_dev", "dc_hip_neighbors_block_pack_wide_dev"),
                        ("dc_hip_neighbors_block_unpack_xwide_dev", "dc_hip_neighbors_block_unpack_wide_dev"),
                        ("dc_hip_xwide_layout_status_dev", "dc_hip_wide_layout_status_dev")):
        getattr(lib, xwide).restype = getattr(lib, wide).restype     # (257..1024 columns: the lists of their namesakes)
        getattr(lib, xwide).argtypes = getattr(lib, wide).argtypes
    lib.dc_hip_session_open_flags.restype = i32
    lib.dc_hip_session_open_flags.argtypes = [vp, sz, sz, C.POINTER(C.c_int), i32, C.c_uint, C.POINTER(vp)]
    lib.dc_hip_session_wide.restype = i32
    lib.dc_hip_session_wide.argtypes = [vp]
    # the three resident reference handles (wide: 65..256 columns, xwide: 257..1024, narrow: 1..64): one list per step, and the three that differ
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    for api, open_extra, third_counter, order_extra in (("dc_hip_reference_wide_", [], u64p, []),
                                                        ("dc_hip_reference_xwide_", [], u64p, []),   # (257..1024 columns)
                                                        ("dc_hip_reference_", [C.c_float], u32p, [i32])):
        for step, restype, argtypes in (("workspace_bytes", sz, [sz, sz, sz]),
                                        ("open_dev", i32, [vp, sz, sz, sz] + open_extra + [vp, sz, vp, C.POINTER(vp)]),
                                        ("close", None, [vp]),
                                        ("set_free_energies_dev", i32, [vp, vp, vp]),
                                        ("stage_dev", i32, [vp, vp, sz, vp]),
                                        ("populations_dev", i32, [vp, C.POINTER(C.c_float), sz, vp, vp]),
                                        ("nearest_dev", i32, [vp, vp, vp, vp, vp, vp, vp]),
                                        ("info_dev", i32, [vp, u64p, u64p, third_counter, u32p, u32p, vp]),
                                        ("order_dev", i32, [vp] + order_extra + [vp, vp, vp])):
            getattr(lib, api + step).restype = restype
            getattr(lib, api + step).argtypes = argtypes
    lib.dc_hip_assign_workspace_bytes.restype = sz
    lib.dc_hip_assign_workspace_bytes.argtypes = [sz, sz]
    lib.dc_hip_assign_open_dev.restype = i32
    lib.dc_hip_assign_open_dev.argtypes = [vp, vp, C.c_uint32, C.c_float, vp, sz, vp, C.POINTER(vp)]
    lib.dc_hip_assign_open_wide_dev.restype = i32
    lib.dc_hip_assign_open_wide_dev.argtypes = lib.dc_hip_assign_open_dev.argtypes
    lib.dc_hip_assign_open_xwide_dev.restype = i32
    lib.dc_hip_assign_open_xwide_dev.argtypes = lib.dc_hip_assign_open_dev.argtypes
    lib.dc_hip_assign_close.restype = None
    lib.dc_hip_assign_close.argtypes = [vp]
    lib.dc_hip_assign_batch_dev.restype = i32
    lib.dc_hip_assign_batch_dev.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.dc_hip_assigner_open.restype = i32
    lib.dc_hip_assigner_open.argtypes = [vp, sz, sz, vp, C.c_float, sz, i32, C.POINTER(vp)]
    lib.dc_hip_assigner_open_flags.restype = i32
    lib.dc_hip_assigner_open_flags.argtypes = [vp, sz, sz, vp, C.c_float, sz, i32, C.c_uint, C.POINTER(vp)]
    lib.dc_hip_assigner_reference.restype = i32
    lib.dc_hip_assigner_reference.argtypes = [vp, vp, vp, C.POINTER(C.c_uint32)]
    lib.dc_hip_assigner_path.restype = i32
    lib.dc_hip_assigner_path.argtypes = [vp]
    lib.dc_hip_assigner_assign.restype = i32
    lib.dc_hip_assigner_assign.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.dc_hip_assigner_close.restype = None
    lib.dc_hip_assigner_close.argtypes = [vp]
    lib.dc_hip_free_energies_scaled_dev.restype = i32
    lib.dc_hip_free_energies_scaled_dev.argtypes = [vp, sz, C.c_uint32, vp, vp]
    lib.dc_hip_populations_cross.restype = i32
    lib.dc_hip_populations_cross.argtypes = [vp, sz, vp, sz, sz, vp, sz, sz, sz, i32, vp]
    lib.dc_hip_nearest_neighbors_cross.restype = i32
    lib.dc_hip_nearest_neighbors_cross.argtypes = [vp, sz, vp, sz, sz, vp, vp, sz, sz, i32, vp, vp, vp, vp]
    return lib


lib = _load()


def check(rc, what=""):
    if rc != DC_OK:
        msg = lib.dc_hip_last_error().decode("utf-8", "replace")
        err = DensityLibraryError(f"{what or 'dc_hip call'} failed (status {rc}): {msg}")
        err.status, err.detail = int(rc), msg
        raise err


def device_count():
    n = lib.dc_hip_device_count()
    if n < 0:
        check(n, "dc_hip_device_count")
    return n
