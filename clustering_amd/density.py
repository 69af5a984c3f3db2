"""Host-side Python mirror of the reference's density hot-path interface
(Clustering::Density::CUDA::*, density_clustering_cuda.hpp:13-54) over the C ABI.

torch is used here only as plumbing: device memory (tensors), streams and, in
clustering_amd.distributed, torch.distributed.  All compute goes through
libdcdensity.so; nothing in this package computes distances on the CPU or in torch.
"""
import ctypes as C
import functools

import numpy as np
import torch

from . import capi
from .rows import shard_rows  # noqa: F401  (re-export)

FLT_MAX = float(np.finfo(np.float32).max)


def get_num_gpus():
    """Clustering::Density::CUDA::get_num_gpus (density_clustering_cuda.cu:32-43): raises if none."""
    n = capi.device_count()
    if n == 0:
        raise capi.DensityLibraryError("error: no HIP-compatible GPUs found")
    return n


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t):
    return C.c_void_p(t.data_ptr())


# The cached workspaces, by kind: the library's byte count for a call's shape -- (n_rows, n_cols[, n_radii]) for the self
# sweeps, (n_q, n_ref, n_cols[, n_radii]) for the sweeps against a reference.  A new kind of sweep is one more row.
_SIZES = {
    "self": capi.lib.dc_hip_workspace_bytes,
    "cross": lambda n_q, n_ref, n_cols, n_radii=1: capi.lib.dc_hip_cross_workspace_bytes(n_q, n_ref, n_cols),
    # ... of variant="cross_pruned" (the larger layout of its two orders)
    "cross_pruned": lambda n_q, n_ref, n_cols, n_radii=1: capi.lib.dc_hip_cross_workspace_bytes_for(
        n_q, n_ref, n_cols, capi.VARIANT_CROSS_PRUNED),
    # ... of nearest_reference(pruned=True)
    "nearest_pruned": lambda n_q, n_ref, n_cols, n_radii=1: capi.lib.dc_hip_nearest_cross_pruned_workspace_bytes(n_q, n_ref, n_cols),
    # the matrix-core sweeps for rows of 65..256 columns, their pruned form, their cross form and its pruned form
    "wide": capi.lib.dc_hip_wide_workspace_bytes,
    "wide_pruned": capi.lib.dc_hip_wide_pruned_workspace_bytes,
    "wide_against": capi.lib.dc_hip_cross_wide_workspace_bytes,
    "wide_against_pruned": capi.lib.dc_hip_cross_wide_pruned_workspace_bytes,
    # ... and the unpruned self and cross sweeps for rows of 257..1024 columns (a layout of their own)
    "xwide": capi.lib.dc_hip_xwide_workspace_bytes,
    "xwide_against": capi.lib.dc_hip_cross_xwide_workspace_bytes,
    # ... and their pruned self sweeps
    "xwide_pruned": capi.lib.dc_hip_xwide_pruned_workspace_bytes,
    # ... and their pruned cross sweeps
    "xwide_against_pruned": capi.lib.dc_hip_cross_xwide_pruned_workspace_bytes,
    # the fp32-input matrix-core sweeps for rows of 1..32 columns
    "fp32": capi.lib.dc_hip_fp32_workspace_bytes,
}


class Workspace:
    """Device scratch of one kind of sweep (MFMA operand images); grown on demand, reused across calls.
    ``size`` is the library's byte count for a call's shape: get(*shape) asks it and returns (pointer, bytes)."""

    def __init__(self, device, size=_SIZES["self"]):
        self.device = device
        self.size = size
        self.buf = None

    def get(self, *shape):
        need = int(self.size(*shape))
        if need == 0:
            return C.c_void_p(0), 0
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        return _dev(self.buf), int(self.buf.numel())


_caches = {kind: {} for kind in _SIZES}   # kind -> device -> Workspace
_shapes = {kind: {} for kind in _SIZES}   # kind -> device -> the shape of the last call that passed capi.check (the pruned
#                                           wide kinds record it: their order readers ask the library for that shape)


def _cached(kind, device):
    key = str(device)
    if key not in _caches[kind]:
        _caches[kind][key] = Workspace(device, _SIZES[kind])
    return _caches[kind][key]


def _get(kind, device, *shape):
    """(pointer, bytes) of the cached workspace of one kind for a call's shape.  A cross-wide call with an empty side needs
    no workspace; it gets the cached buffer, if there is one, so that the info reader of its kind reports that nothing was
    swept rather than the call before."""
    cache = _cached(kind, device)
    ws, ws_bytes = cache.get(*shape)
    if ws_bytes == 0 and cache.buf is not None and kind in ("wide_against", "wide_against_pruned", "xwide_against"):
        return _dev(cache.buf), int(cache.buf.numel())
    return ws, ws_bytes


# (the names tests and tools reach into: lookups into the registry)
_workspace = functools.partial(_cached, "self")
_cross_workspace = functools.partial(_cached, "cross")
_cross_pruned_workspace = functools.partial(_cached, "cross_pruned")
_wide_workspace = functools.partial(_cached, "wide")
_wide_pruned_workspace = functools.partial(_cached, "wide_pruned")
_wide_against_pruned_workspace = functools.partial(_cached, "wide_against_pruned")
_cross_pruned_workspaces = _caches["cross_pruned"]
_nearest_pruned_workspaces = _caches["nearest_pruned"]


def _variant(variant, stats_valid):
    """the C ABI's `variant` argument: kernel family | DC_FLAG_STATS_VALID (the workspace header still holds the
    statistics of an earlier sweep over the SAME coordinates: the second call of a populations -> neighbours pair)"""
    return capi.VARIANTS[variant] | (capi.FLAG_STATS_VALID if stats_valid else 0)


def _check_coords(coords):
    if not (isinstance(coords, torch.Tensor) and coords.is_cuda and coords.dtype == torch.float32
            and coords.dim() == 2 and coords.is_contiguous()):
        raise ValueError("coords must be a contiguous float32 CUDA tensor [n_rows, n_cols]")
    return coords.shape[0], coords.shape[1]


def _ascending(rad, out):
    """Several radii go to the library in ASCENDING order (the symmetric multi-radius sweep then leaves out the small
    radii a tile pair holds nothing of -- INTEGRATION.md section 5); the rows come back in the caller's order.
    -> (radii for the call, buffer for the call, row permutation or None)"""
    if rad.size < 2 or bool(np.all(rad[1:] >= rad[:-1])):
        return rad, out, None
    order = np.argsort(rad, kind="stable")
    return np.ascontiguousarray(rad[order]), torch.empty_like(out), torch.from_numpy(order).to(out.device)


def _populations(fn, kind, device, head, sizes, radii, span, out, variant=None, ascending=False):
    """One population call of the library function ``fn`` in the cached workspace of ``kind``.  head: the leading C
    arguments (the arrays and their sizes); sizes: the shape the workspace is sized for, the rows of the result first;
    span: the row range or the segment; variant: the C ``variant`` argument of the calls that take one.  Only the narrow
    calls reorder their radii (ascending=True); the others pass the caller's order.  -> int32 [n_radii, sizes[0]]"""
    rad = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
    if out is None:
        out = torch.empty((rad.size, sizes[0]), dtype=torch.int32, device=device)
    assert out.shape == (rad.size, sizes[0]) and out.dtype == torch.int32 and out.is_contiguous()
    rad_call, dst, order = _ascending(rad, out) if ascending else (rad, out, None)
    with torch.cuda.device(device):
        ws, ws_bytes = _get(kind, device, *sizes, rad.size)
        rc = getattr(capi.lib, fn)(*head, rad_call.ctypes.data_as(C.POINTER(C.c_float)), rad.size, *span, _dev(dst), ws, ws_bytes,
                                   *(() if variant is None else (variant,)), _stream_ptr())
    capi.check(rc, fn)
    if order is not None:
        out[order] = dst
    return out


def _neighbors(fn, kind, coords, fe, span, variant=None):
    """One self-neighbour call of ``fn`` in the cached workspace of ``kind``, like _populations; a row range may leave its
    end open (None: n_rows).  -> (nn_idx int32, nn_d2 float32, hd_idx int32, hd_d2 float32), each [n_rows]"""
    n_rows, n_cols = _check_coords(coords)
    span = (span[0], n_rows if span[1] is None else span[1])
    assert fe.is_cuda and fe.dtype == torch.float32 and fe.shape == (n_rows,) and fe.is_contiguous()
    dev = coords.device
    nn_idx = torch.empty(n_rows, dtype=torch.int32, device=dev)
    hd_idx = torch.empty(n_rows, dtype=torch.int32, device=dev)
    nn_d2 = torch.empty(n_rows, dtype=torch.float32, device=dev)
    hd_d2 = torch.empty(n_rows, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws, ws_bytes = _get(kind, dev, n_rows, n_cols, 1)
        rc = getattr(capi.lib, fn)(_dev(coords), n_rows, n_cols, _dev(fe), *span, _dev(nn_idx), _dev(nn_d2), _dev(hd_idx),
                                   _dev(hd_d2), ws, ws_bytes, *(() if variant is None else (variant,)), _stream_ptr())
    capi.check(rc, fn)
    return nn_idx, nn_d2, hd_idx, hd_d2


def calculate_populations_partial(coords, radii, i_from=0, i_to=None, variant="auto", out=None, stats_valid=False):
    """Per-GPU partial of calculate_populations (density_clustering_cuda.cu:45-137).

    coords: float32 CUDA tensor [n_rows, n_cols]; radii: sequence of float.
    -> torch.int32 [n_radii, n_rows] (the ABI's uint32 bit pattern; populations are <= n_rows
    < 2^31 whenever the tensor itself is addressable), radius-major in the order of ``radii``,
    zero outside [i_from, i_to).
    """
    n_rows, n_cols = _check_coords(coords)
    return _populations("dc_hip_populations_dev", "self", coords.device, (_dev(coords), n_rows, n_cols), (n_rows, n_cols), radii,
                        (i_from, n_rows if i_to is None else i_to), out, _variant(variant, stats_valid), ascending=True)


def calculate_populations_segment(coords, radii, segment, n_segments, variant="auto", out=None, stats_valid=False):
    """Populations of one segment of a sharded run (dc_hip_populations_segment_dev): with the pruned
    sweep every n_segments-th query group of the spatial order, else the reference's row block.  PARTIAL counts
    that merge by summation over the segments (a one-radius pruned sweep is symmetric -- it credits both frames
    of a pair -- so a segment's counts cover all rows; the other sweeps leave zeros outside the segment)."""
    n_rows, n_cols = _check_coords(coords)
    return _populations("dc_hip_populations_segment_dev", "self", coords.device, (_dev(coords), n_rows, n_cols), (n_rows, n_cols),
                        radii, (segment, n_segments), out, _variant(variant, stats_valid), ascending=True)


def nearest_neighbors_segment(coords, fe, segment, n_segments, variant="auto", stats_valid=False):
    """Neighbours of one segment of a sharded run (dc_hip_nearest_neighbors_segment_dev); the rows of
    other segments hold (n_rows+1, FLT_MAX)."""
    return _neighbors("dc_hip_nearest_neighbors_segment_dev", "self", coords, fe, (segment, n_segments),
                      _variant(variant, stats_valid))


def calculate_free_energies(pops):
    """calculate_free_energies (density_clustering.cpp:197-212) for one radius. pops: int32 CUDA [n_rows]."""
    assert pops.is_cuda and pops.dtype == torch.int32 and pops.dim() == 1 and pops.is_contiguous()
    fe = torch.empty(pops.shape[0], dtype=torch.float32, device=pops.device)
    mx = C.c_uint32(0)
    with torch.cuda.device(pops.device):
        rc = capi.lib.dc_hip_free_energies_dev(_dev(pops), pops.shape[0], _dev(fe), C.byref(mx),
                                               _stream_ptr())
    capi.check(rc, "dc_hip_free_energies_dev")
    return fe


def nearest_neighbors_partial(coords, fe, i_from=0, i_to=None, variant="auto", stats_valid=False):
    """Per-GPU partial of nearest_neighbors (density_clustering_cuda.cu:184-284).

    -> (nn_idx int32, nn_d2 float32, hd_idx int32, hd_d2 float32), each [n_rows]; rows outside the
    range hold the reference's "none" value (n_rows+1, FLT_MAX)."""
    return _neighbors("dc_hip_nearest_neighbors_dev", "self", coords, fe, (i_from, i_to), _variant(variant, stats_valid))


# ---- matrix-core sweeps for rows of 65..256 columns (include/dc_density.h "wide" sweeps) ---------------------------
def calculate_populations_wide(coords, radii, i_from=0, i_to=None, out=None):
    """calculate_populations_partial for rows of 65..256 columns on the matrix cores (dc_hip_populations_wide_dev):
    the same populations bit for bit, one matrix-core chain per tile pair for all radii (up to 8 per launch), radii in
    any order, in a cached workspace of its own (wide_sweep_info reads its counters).  Other column counts raise."""
    n_rows, n_cols = _check_coords(coords)
    return _populations("dc_hip_populations_wide_dev", "wide", coords.device, (_dev(coords), n_rows, n_cols), (n_rows, n_cols),
                        radii, (i_from, n_rows if i_to is None else i_to), out)


def nearest_neighbors_wide(coords, fe, i_from=0, i_to=None):
    """nearest_neighbors_partial for rows of 65..256 columns on the matrix cores (dc_hip_nearest_neighbors_wide_dev).
    -> (nn_idx int32, nn_d2 float32, hd_idx int32, hd_d2 float32), each [n_rows]; "none" is (n_rows+1, FLT_MAX)."""
    return _neighbors("dc_hip_nearest_neighbors_wide_dev", "wide", coords, fe, (i_from, i_to))


# ---- fp32-input matrix-core sweeps for rows of 1..32 columns (include/dc_density.h "fp32" sweeps) -----------------
def calculate_populations_fp32(coords, radii, i_from=None, i_to=None):
    """calculate_populations_partial on the fp32-input matrix cores (dc_hip_populations_fp32_dev) for rows of 1..32
    columns: the same populations bit for bit, every pair evaluated, up to 8 radii of the call sharing one pass of the
    MFMAs (fp32_sweep_plan says how a call is run); radii in any order.  Other column counts raise.
    -> torch.int32 [n_radii, n_rows], zero outside [i_from, i_to)."""
    n_rows, n_cols = _check_coords(coords)
    return _populations("dc_hip_populations_fp32_dev", "fp32", coords.device, (_dev(coords), n_rows, n_cols), (n_rows, n_cols),
                        radii, (0 if i_from is None else i_from, n_rows if i_to is None else i_to), None)


def nearest_neighbors_fp32(coords, fe, i_from=None, i_to=None):
    """nearest_neighbors_partial on the fp32-input matrix cores (dc_hip_nearest_neighbors_fp32_dev), 1..32 columns.
    -> (nn_idx int32, nn_d2 float32, hd_idx int32, hd_d2 float32), each [n_rows]; "none" is (n_rows+1, FLT_MAX)."""
    return _neighbors("dc_hip_nearest_neighbors_fp32_dev", "fp32", coords, fe, (0 if i_from is None else i_from, i_to))


def fp32_sweep_plan(n_rows, n_cols, n_radii):
    """How the fp32 sweeps run a call of this shape (dc_hip_fp32_plan; decided on the host, no device needed) -> dict:
    k_steps (MFMAs per chain: ceil(n_cols / 2), at some widths one zero step more), lane_floats (floats per lane and
    tile of the operand image), tq_pop / tq_nn (query tiles per wave), radii_per_sweep, sweeps, chunks_pop / chunks_nn
    (reference chunks), lds_pop / lds_nn (dynamic LDS bytes per workgroup), image_bytes_per_tile and
    image_region_bytes_per_tile (what the workspace keeps for it)."""
    out = (C.c_uint32 * 8)()
    capi.check(capi.lib.dc_hip_fp32_plan(n_rows, n_cols, n_radii, out), "dc_hip_fp32_plan")
    w = [int(v) for v in out]
    return {"k_steps": w[0], "lane_floats": w[1], "tq_pop": w[2] & 0xFFFF, "tq_nn": w[2] >> 16,
            "radii_per_sweep": w[3] & 0xFFFF, "sweeps": w[3] >> 16, "chunks_pop": w[4] & 0xFFFF, "chunks_nn": w[4] >> 16,
            "lds_pop": w[5], "lds_nn": w[6], "image_bytes_per_tile": w[7] & 0xFFFF, "image_region_bytes_per_tile": w[7] >> 16}


def _wide_info(kind, device):
    """(tiles, mfmas, exact_pairs) from the head of this device's workspace of ``kind`` (dc_hip_wide_info_dev)"""
    ws = _cached(kind, device)
    if ws.buf is None:
        return 0, 0, 0
    t, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    with torch.cuda.device(device):
        capi.check(capi.lib.dc_hip_wide_info_dev(_dev(ws.buf), C.byref(t), C.byref(m), C.byref(e), _stream_ptr()),
                   "dc_hip_wide_info_dev")
    return int(t.value), int(m.value), int(e.value)


def wide_sweep_info(device):
    """(tiles, mfmas, exact_pairs): 32x32 frame-pair tiles evaluated, MFMA instructions issued and frame pairs sent
    to the exact path by the last wide sweep on this device (dc_hip_wide_info_dev); (0, 0, 0) when the direct
    kernels answered (flagged data), nothing was swept, or no wide sweep has run."""
    return _wide_info("wide", device)


# ---- ... and for rows of 257..1024 columns (include/dc_density.h, the "extra-wide" sweeps) ---------------------------
def calculate_populations_xwide(coords, radii, i_from=0, i_to=None, out=None):
    """calculate_populations_wide for rows of 257..1024 columns (dc_hip_populations_xwide_dev): the same kernel over a
    longer chain, the same populations bit for bit as variant="direct", in a cached workspace of its own kind
    (xwide_sweep_info reads its counters).  Other column counts raise."""
    n_rows, n_cols = _check_coords(coords)
    return _populations("dc_hip_populations_xwide_dev", "xwide", coords.device, (_dev(coords), n_rows, n_cols), (n_rows, n_cols),
                        radii, (i_from, n_rows if i_to is None else i_to), out)


def nearest_neighbors_xwide(coords, fe, i_from=0, i_to=None):
    """nearest_neighbors_wide for rows of 257..1024 columns (dc_hip_nearest_neighbors_xwide_dev).
    -> (nn_idx int32, nn_d2 float32, hd_idx int32, hd_d2 float32), each [n_rows]; "none" is (n_rows+1, FLT_MAX)."""
    return _neighbors("dc_hip_nearest_neighbors_xwide_dev", "xwide", coords, fe, (i_from, i_to))


def xwide_sweep_info(device):
    """(tiles, mfmas, exact_pairs) of the last calculate_populations_xwide / nearest_neighbors_xwide on this device, as
    wide_sweep_info gives them; (0, 0, 0) when the direct kernels answered (flagged data), nothing was swept, or no such
    sweep has run."""
    return _wide_info("xwide", device)


# ---- ... and their pruned self sweeps (include/dc_density.h, the PRUNED sweeps at 257..1024 columns) -----------------
def calculate_populations_xwide_pruned(coords, radii, segment=0, n_segments=0, out=None):
    """calculate_populations_wide_pruned for rows of 257..1024 columns (dc_hip_populations_xwide_pruned_dev): the
    populations of calculate_populations_xwide and of variant="direct" bit for bit, without the block pairs that cannot
    hold a pair within the radii.  Segments as calculate_populations_wide_pruned takes them.  In a cached workspace of its
    own kind (xwide_pruned_info reads its counters, xwide_pruned_order its order).  Other column counts raise."""
    n_rows, n_cols = _check_coords(coords)
    out = _populations("dc_hip_populations_xwide_pruned_dev", "xwide_pruned", coords.device, (_dev(coords), n_rows, n_cols),
                       (n_rows, n_cols), radii, (segment, n_segments), out)
    _shapes["xwide_pruned"][str(coords.device)] = (n_rows, n_cols)
    return out


def nearest_neighbors_xwide_pruned(coords, fe, segment=0, n_segments=0):
    """nearest_neighbors_wide_pruned for rows of 257..1024 columns (dc_hip_nearest_neighbors_xwide_pruned_dev): the four
    arrays of nearest_neighbors_xwide bit for bit.  In the cached workspace of calculate_populations_xwide_pruned."""
    out = _neighbors("dc_hip_nearest_neighbors_xwide_pruned_dev", "xwide_pruned", coords, fe, (segment, n_segments))
    _shapes["xwide_pruned"][str(coords.device)] = tuple(coords.shape)
    return out


def xwide_pruned_info(device):
    """(tiles, mfmas, exact_pairs) of the last pruned sweep of 257..1024 columns on this device, as wide_pruned_info gives
    them: the EVALUATED tile pairs; (0, 0, 0) when the direct kernel answered (flagged data), the segment held no block, or
    no such sweep has run."""
    return _wide_info("xwide_pruned", device)


def xwide_pruned_order(device):
    """the spatial order of the last pruned sweep of 257..1024 columns on this device: int32 [n_rows], position -> row
    (dc_hip_xwide_pruned_order_dev)."""
    return _pruned_order("xwide_pruned", "dc_hip_xwide_pruned_order_dev", device)


# ---- ... the pruned self population sweep (include/dc_density.h, the PRUNED wide sweep) ------------------------------
def calculate_populations_wide_pruned(coords, radii, segment=0, n_segments=0, out=None):
    """calculate_populations_wide without the block pairs that cannot hold a pair within the radii
    (dc_hip_populations_wide_pruned_dev): the same populations bit for bit.  n_segments == 0: the whole sweep (segment is not read);
    otherwise the query blocks segment, segment + n_segments, ... of the spatial order (wide_pruned_order): final counts
    for their rows, zeros elsewhere.  In a cached workspace of its own (wide_pruned_info reads its counters)."""
    n_rows, n_cols = _check_coords(coords)
    out = _populations("dc_hip_populations_wide_pruned_dev", "wide_pruned", coords.device, (_dev(coords), n_rows, n_cols),
                       (n_rows, n_cols), radii, (segment, n_segments), out)
    _shapes["wide_pruned"][str(coords.device)] = (n_rows, n_cols)
    return out


def nearest_neighbors_wide_pruned(coords, fe, segment=0, n_segments=0):
    """nearest_neighbors_wide in the spatial order of the pruned wide sweeps, searching outward and stopping
    (dc_hip_nearest_neighbors_wide_pruned_dev): the same four arrays bit for bit.  n_segments == 0: the whole sweep
    (segment is not read); otherwise the query blocks segment, segment + n_segments, ... of the order
    (wide_pruned_order): final results on their rows, "none" elsewhere.  In the cached workspace of the pruned wide
    sweeps (wide_pruned_info reads its counters, wide_pruned_order its order)."""
    out = _neighbors("dc_hip_nearest_neighbors_wide_pruned_dev", "wide_pruned", coords, fe, (segment, n_segments))
    _shapes["wide_pruned"][str(coords.device)] = tuple(coords.shape)
    return out


def wide_pruned_info(device):
    """(tiles, mfmas, exact_pairs) of the last calculate_populations_wide_pruned on this device, as wide_sweep_info
    gives them; the tile pairs are the evaluated ones.  (0, 0, 0) when the direct kernel answered (flagged data), the
    segment held no block, or no such sweep has run."""
    return _wide_info("wide_pruned", device)


def wide_pruned_order(device):
    """the spatial order of the last calculate_populations_wide_pruned on this device: int32 [n_rows], position -> row
    (block b of the order: positions 128 b .. 128 b + 127) (dc_hip_wide_pruned_order_dev)."""
    return _pruned_order("wide_pruned", "dc_hip_wide_pruned_order_dev", device)


def _pruned_order(kind, fn, device):
    """the order reader of a pruned self kind: the library's ``fn`` for the shape of the last call in that workspace"""
    ws, shape = _cached(kind, device), _shapes[kind].get(str(device))
    if ws.buf is None or shape is None:
        raise ValueError("no pruned wide sweep has run on this device")
    perm = torch.empty(shape[0], dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        capi.check(getattr(capi.lib, fn)(_dev(ws.buf), shape[0], shape[1], _dev(perm), _stream_ptr()), fn)
    return perm


# ---- cross sweeps: new frames against a reference trajectory (include/dc_density.h "cross sweeps") ----------------
def _check_pair(queries, reference):
    n_q, n_cols = _check_coords(queries)
    n_ref, n_cols_r = _check_coords(reference)
    if n_cols != n_cols_r or queries.device != reference.device:
        raise ValueError("queries and reference need the same n_cols and the same device")
    return n_q, n_ref, n_cols


def _populations_against(fn, kind, queries, reference, sizes, radii, i_from, i_to, out, variant=None, ascending=False):
    """_populations for the query frames [i_from, i_to) in a reference; sizes: (n_q, n_ref, n_cols), checked by the caller"""
    n_q, n_ref, n_cols = sizes
    return _populations(fn, kind, queries.device, (_dev(queries), n_q, _dev(reference), n_ref, n_cols), sizes, radii,
                        (i_from, n_q if i_to is None else i_to), out, variant, ascending)


def _nearest(fn, kind, queries, reference, sizes, fe_query, fe_ref, i_from, i_to, variant=None):
    """One cross-neighbour call of ``fn`` in the cached workspace of ``kind``; sizes: (n_q, n_ref, n_cols), checked by the
    caller.  -> (nn_idx int32, nn_d2 float32, hd_idx, hd_d2), each [n_q]; without free energies hd_idx / hd_d2 are None"""
    n_q, n_ref, n_cols = sizes
    i_to = n_q if i_to is None else i_to
    with_fe = fe_query is not None
    if with_fe:
        assert fe_ref is not None
        for f, n in ((fe_query, n_q), (fe_ref, n_ref)):
            assert f.is_cuda and f.dtype == torch.float32 and f.shape == (n,) and f.is_contiguous()
    dev = queries.device
    nn_idx = torch.empty(n_q, dtype=torch.int32, device=dev)
    nn_d2 = torch.empty(n_q, dtype=torch.float32, device=dev)
    hd_idx = torch.empty(n_q, dtype=torch.int32, device=dev) if with_fe else None
    hd_d2 = torch.empty(n_q, dtype=torch.float32, device=dev) if with_fe else None
    with torch.cuda.device(dev):
        ws, ws_bytes = _get(kind, dev, n_q, n_ref, n_cols, 1)
        rc = getattr(capi.lib, fn)(
            _dev(queries), n_q, _dev(reference), n_ref, n_cols, _dev(fe_query) if with_fe else None,
            _dev(fe_ref) if with_fe else None, i_from, i_to, _dev(nn_idx), _dev(nn_d2),
            _dev(hd_idx) if with_fe else None, _dev(hd_d2) if with_fe else None, ws, ws_bytes,
            *(() if variant is None else (variant,)), _stream_ptr())
    capi.check(rc, fn)
    return nn_idx, nn_d2, hd_idx, hd_d2


def calculate_populations_against(queries, reference, radii, i_from=0, i_to=None, variant="auto", out=None):
    """Populations of the query frames in the reference trajectory (dc_hip_populations_cross_dev):
    pops[r][q] = #{ j : d2(Q_q, R_j) < r^2 } -- no self term, so a copy of reference frame j gets pop_R(j).
    queries [n_q, n_cols], reference [n_ref, n_cols]: float32 CUDA tensors; radii in any order.
    -> torch.int32 [n_radii, n_q] in the order of ``radii``, zero outside [i_from, i_to).
    variant="cross_pruned" (n_cols <= 64): the matrix-core sweep with tile-pair pruning, in a workspace of its own
    (evaluated_tiles_against reads its counters); the same results."""
    return _populations_against("dc_hip_populations_cross_dev", "cross_pruned" if variant == "cross_pruned" else "cross", queries,
                                reference, _check_pair(queries, reference), radii, i_from, i_to, out, capi.VARIANTS[variant],
                                ascending=True)


def calculate_free_energies_against(pops, max_pop):
    """Free energies on another population array's scale (dc_hip_free_energies_scaled_dev):
    fe = (float)-log((double)((float)pop * (1.0f / max_pop))).  pops: int32 CUDA [n]; pop 0 -> +inf,
    pop > max_pop -> negative."""
    assert pops.is_cuda and pops.dtype == torch.int32 and pops.dim() == 1 and pops.is_contiguous()
    fe = torch.empty(pops.shape[0], dtype=torch.float32, device=pops.device)
    with torch.cuda.device(pops.device):
        rc = capi.lib.dc_hip_free_energies_scaled_dev(_dev(pops), pops.shape[0], int(max_pop), _dev(fe), _stream_ptr())
    capi.check(rc, "dc_hip_free_energies_scaled_dev")
    return fe


def nearest_reference(queries, reference, fe_query=None, fe_ref=None, i_from=0, i_to=None, variant="auto", pruned=False):
    """Nearest reference frame of every query, and nearest reference frame of strictly lower free energy
    (dc_hip_nearest_neighbors_cross_dev).  -> (nn_idx int32, nn_d2 float32, hd_idx, hd_d2), each [n_q]; "none" is
    (n_ref + 1, FLT_MAX).  Without free energies hd_idx / hd_d2 are None.
    pruned=True (n_cols <= 64, variant must be "auto"): the matrix-core sweep that skips the tile pairs which cannot
    matter (dc_hip_nearest_neighbors_cross_pruned_dev), in a cached workspace of its own; the same results bit for bit.
    evaluated_tiles_nearest_reference tells what it evaluated."""
    if pruned and variant != "auto":
        raise ValueError(f"nearest_reference(pruned=True) takes variant='auto', not {variant!r}: the pruned sweep is "
                         "an entry point of its own")
    sizes = _check_pair(queries, reference)
    if pruned:
        return _nearest("dc_hip_nearest_neighbors_cross_pruned_dev", "nearest_pruned", queries, reference, sizes, fe_query, fe_ref,
                        i_from, i_to)
    return _nearest("dc_hip_nearest_neighbors_cross_dev", "cross", queries, reference, sizes, fe_query, fe_ref, i_from, i_to,
                    capi.VARIANTS[variant])


def evaluated_tiles_nearest_reference(device):
    """(nn_tiles, nn_mfma, n_shares): 32x32 frame-pair tiles evaluated, MFMA instructions issued and reference shares of
    the launch of the last nearest_reference(..., pruned=True) on this device (dc_hip_nearest_cross_pruned_info_dev).
    (0, 0, 0) after a call the pruned kernel did not answer: flagged data, a reference beyond 2^24 positions, nothing
    to sweep."""
    ws = _cached("nearest_pruned", device)
    if ws.buf is None:
        return 0, 0, 0
    t, m, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    with torch.cuda.device(device):
        capi.check(capi.lib.dc_hip_nearest_cross_pruned_info_dev(_dev(ws.buf), C.byref(t), C.byref(m), C.byref(n),
                                                                 _stream_ptr()),
                   "dc_hip_nearest_cross_pruned_info_dev")
    return int(t.value), int(m.value), int(n.value)


def _assign_frames(queries, reference, radius, ref_states, sizes, pops_self, pops_against, nearest):
    """the four steps of assign_frames with the three sweeps it is given -> its dict"""
    n_q, n_ref, _ = sizes
    dev = queries.device
    states_r = torch.as_tensor(np.ascontiguousarray(ref_states, dtype=np.int32), device=dev)
    assert states_r.shape == (n_ref,)
    pops_ref = pops_self(reference, [radius])[0].contiguous()
    max_pop = int(pops_ref.max().item()) if n_ref else 0
    fe_ref = calculate_free_energies(pops_ref)
    pops_q = pops_against(queries, reference, [radius])[0].contiguous()
    fe_q = calculate_free_energies_against(pops_q, max_pop) if max_pop else \
        torch.full((n_q,), float("inf"), dtype=torch.float32, device=dev)
    nn_idx, nn_d2, hd_idx, hd_d2 = nearest(queries, reference, fe_q, fe_ref)
    none = n_ref + 1
    states = torch.zeros(n_q, dtype=torch.int32, device=dev)
    if n_ref:
        pick = torch.where(hd_idx != none, hd_idx, nn_idx)
        ok = pick != none
        states[ok] = states_r[pick[ok].long()]
    return {"states": states, "pops_ref": pops_ref, "max_pop": max_pop, "fe_ref": fe_ref, "pops": pops_q, "fe": fe_q,
            "nn_idx": nn_idx, "nn_d2": nn_d2, "hd_idx": hd_idx, "hd_d2": hd_d2}


def assign_frames(queries, reference, radius, ref_states, variant="auto", pruned_neighbours=False):
    """Assign new frames to the states of an already clustered reference trajectory, end to end:
      1. the reference's own populations at ``radius`` (self sweep), their maximum and the reference free energies;
      2. the query populations in the reference and the query free energies on the reference's scale;
      3. nearest reference frame and nearest reference frame of lower free energy;
      4. the state of each query: ref_states[hd] if hd exists, else ref_states[nn], else 0 (unassigned, as in the
         reference's density_clustering.cpp:345-360).
    ref_states: int array-like [n_ref].  -> dict of CUDA tensors (states int32 [n_q] among them).
    variant="cross_pruned": step 2 runs the pruned sweep against the reference; the self sweep of step 1 and the
    neighbours of step 3 run on "auto".  pruned_neighbours=True: step 3 runs the pruned neighbour sweep
    (nearest_reference(pruned=True); the variant must then be "auto" or "cross_pruned").  The two can be combined; the
    results are the same either way."""
    other = "auto" if variant == "cross_pruned" else variant
    return _assign_frames(queries, reference, radius, ref_states, _check_pair(queries, reference),
                          functools.partial(calculate_populations_partial, variant=other),
                          functools.partial(calculate_populations_against, variant=variant),
                          functools.partial(nearest_reference, variant=other, pruned=pruned_neighbours))


# ---- the cross sweeps for rows of 65..256 columns on the matrix cores (include/dc_density.h, the wide sweeps' cross form) ----
def _check_pair_wide(queries, reference):
    """_check_pair, the column count (refused here as the library refuses it: 65..256) first"""
    for t in (queries, reference):
        if isinstance(t, torch.Tensor) and t.dim() == 2 and not 65 <= t.shape[1] <= 256:
            raise ValueError(f"n_cols={t.shape[1]}: the wide matrix-core sweeps take 65..256 columns")
    return _check_pair(queries, reference)


def calculate_populations_against_wide(queries, reference, radii, i_from=0, i_to=None, out=None):
    """calculate_populations_against(variant="direct") for rows of 65..256 columns on the matrix cores
    (dc_hip_populations_cross_wide_dev): the same populations bit for bit -- no self term -- with one matrix-core chain
    per tile pair for all radii (up to 8 per launch), radii in any order, in a cached workspace of its own
    (wide_against_info reads its counters).  Other column counts raise."""
    return _populations_against("dc_hip_populations_cross_wide_dev", "wide_against", queries, reference,
                                _check_pair_wide(queries, reference), radii, i_from, i_to, out)


def nearest_reference_wide(queries, reference, fe_query=None, fe_ref=None, i_from=0, i_to=None):
    """nearest_reference(variant="direct") for rows of 65..256 columns on the matrix cores
    (dc_hip_nearest_neighbors_cross_wide_dev).  -> (nn_idx int32, nn_d2 float32, hd_idx, hd_d2), each [n_q]; "none" is
    (n_ref + 1, FLT_MAX).  Without free energies hd_idx / hd_d2 are None.  Other column counts raise."""
    return _nearest("dc_hip_nearest_neighbors_cross_wide_dev", "wide_against", queries, reference,
                    _check_pair_wide(queries, reference), fe_query, fe_ref, i_from, i_to)


def wide_against_info(device):
    """(tiles, mfmas, exact_pairs) of the last calculate_populations_against_wide / nearest_reference_wide on this
    device, as wide_sweep_info gives them for the self sweeps (dc_hip_wide_info_dev on the cross sweeps' own workspace);
    (0, 0, 0) when the direct kernels answered (flagged data), nothing was swept, or no such sweep has run."""
    return _wide_info("wide_against", device)


# ---- ... and for rows of 257..1024 columns (include/dc_density.h, the "extra-wide" sweeps) ---------------------------
def _check_pair_xwide(queries, reference):
    """_check_pair, the column count (refused here as the library refuses it: 257..1024) first"""
    for t in (queries, reference):
        if isinstance(t, torch.Tensor) and t.dim() == 2 and not 257 <= t.shape[1] <= 1024:
            raise ValueError(f"n_cols={t.shape[1]}: the extra-wide matrix-core sweeps take 257..1024 columns")
    return _check_pair(queries, reference)


def calculate_populations_against_xwide(queries, reference, radii, i_from=0, i_to=None, out=None):
    """calculate_populations_against_wide for rows of 257..1024 columns (dc_hip_populations_cross_xwide_dev), in a cached
    workspace of its own kind (xwide_against_info reads its counters).  Other column counts raise."""
    return _populations_against("dc_hip_populations_cross_xwide_dev", "xwide_against", queries, reference,
                                _check_pair_xwide(queries, reference), radii, i_from, i_to, out)


def nearest_reference_xwide(queries, reference, fe_query=None, fe_ref=None, i_from=0, i_to=None):
    """nearest_reference_wide for rows of 257..1024 columns (dc_hip_nearest_neighbors_cross_xwide_dev).  Without free
    energies hd_idx / hd_d2 are None.  Other column counts raise."""
    return _nearest("dc_hip_nearest_neighbors_cross_xwide_dev", "xwide_against", queries, reference,
                    _check_pair_xwide(queries, reference), fe_query, fe_ref, i_from, i_to)


def xwide_against_info(device):
    """(tiles, mfmas, exact_pairs) of the last calculate_populations_against_xwide / nearest_reference_xwide on this
    device, as wide_against_info gives them."""
    return _wide_info("xwide_against", device)


def assign_frames_xwide(queries, reference, radius, ref_states):
    """assign_frames for rows of 257..1024 columns, every sweep on the matrix cores: calculate_populations_xwide on the
    reference, calculate_populations_against_xwide and nearest_reference_xwide for the queries; the same dict, the same
    values."""
    return _assign_frames(queries, reference, radius, ref_states, _check_pair_xwide(queries, reference), calculate_populations_xwide,
                          calculate_populations_against_xwide, nearest_reference_xwide)


# ---- ... the pruned cross population sweep (include/dc_density.h, the PRUNED wide cross sweep) -----------------------
def _record_against_pruned(queries, sizes, i_from, i_to, kind="wide_against_pruned"):
    """(rows of the query range, n_ref, n_cols) of a pruned wide cross call that passed: what its order reader asks for"""
    n_q, n_ref, n_cols = sizes
    _shapes[kind][str(queries.device)] = (max((n_q if i_to is None else i_to) - i_from, 0), n_ref, n_cols)


def calculate_populations_against_wide_pruned(queries, reference, radii, i_from=0, i_to=None, out=None):
    """calculate_populations_against_wide without the block pairs that cannot hold a pair within the radii
    (dc_hip_populations_cross_wide_pruned_dev): the same populations bit for bit.  The queries [i_from, i_to) and the
    reference are put into one spatial order each, on one cell grid.  In a cached workspace of its own
    (wide_against_pruned_info reads its counters, wide_against_pruned_order its two orders)."""
    sizes = _check_pair_wide(queries, reference)
    out = _populations_against("dc_hip_populations_cross_wide_pruned_dev", "wide_against_pruned", queries, reference, sizes, radii,
                               i_from, i_to, out)
    _record_against_pruned(queries, sizes, i_from, i_to)
    return out


def nearest_reference_wide_pruned(queries, reference, fe_query=None, fe_ref=None, i_from=0, i_to=None):
    """nearest_reference_wide without the block pairs that cannot hold a nearest reference frame
    (dc_hip_nearest_neighbors_cross_wide_pruned_dev): the same four arrays bit for bit.  A query block meets the reference
    block nearest to it first, then the blocks within the bound of its nearest frames, then those within the bound of its
    nearest frames of lower free energy.  In the cached workspace of calculate_populations_against_wide_pruned
    (wide_against_pruned_info reads its counters, wide_against_pruned_order its two orders)."""
    sizes = _check_pair_wide(queries, reference)
    out = _nearest("dc_hip_nearest_neighbors_cross_wide_pruned_dev", "wide_against_pruned", queries, reference, sizes, fe_query,
                   fe_ref, i_from, i_to)
    _record_against_pruned(queries, sizes, i_from, i_to)
    return out


def wide_against_pruned_info(device):
    """(tiles, mfmas, exact_pairs) of the last calculate_populations_against_wide_pruned / nearest_reference_wide_pruned
    on this device (for the neighbour call: summed over its launches), as
    wide_against_info gives them; the tile pairs are the evaluated ones.  (0, 0, 0) when the direct kernel answered
    (flagged data), nothing was swept, or no such sweep has run."""
    return _wide_info("wide_against_pruned", device)


def wide_against_pruned_order(device):
    """both spatial orders of the last calculate_populations_against_wide_pruned / nearest_reference_wide_pruned on this
    device, position -> row:
    (perm_q int32 [i_to - i_from], rows of the queries; perm_r int32 [n_ref]); block b of either order is its
    positions 128 b .. 128 b + 127 (dc_hip_cross_wide_pruned_order_dev)."""
    return _against_pruned_order("wide_against_pruned", "dc_hip_cross_wide_pruned_order_dev", device)


def _against_pruned_order(kind, fn, device):
    """the order reader of a pruned cross kind: the library's ``fn`` for the shape of the last call in that workspace"""
    ws, shape = _cached(kind, device), _shapes[kind].get(str(device))
    if ws.buf is None or shape is None:
        raise ValueError("no pruned wide cross sweep has run on this device")
    perm_q = torch.empty(shape[0], dtype=torch.int32, device=device)
    perm_r = torch.empty(shape[1], dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        capi.check(getattr(capi.lib, fn)(_dev(ws.buf), shape[0], shape[1], shape[2], _dev(perm_q), _dev(perm_r), _stream_ptr()), fn)
    return perm_q, perm_r


def assign_frames_wide(queries, reference, radius, ref_states):
    """assign_frames for rows of 65..256 columns, every sweep on the matrix cores: calculate_populations_wide on the
    reference, calculate_populations_against_wide and nearest_reference_wide for the queries; the same four steps, the
    same state rule, the same dict, the same values."""
    return _assign_frames(queries, reference, radius, ref_states, _check_pair_wide(queries, reference), calculate_populations_wide,
                          calculate_populations_against_wide, nearest_reference_wide)


def assign_frames_wide_pruned(queries, reference, radius, ref_states, pruned_neighbours=False):
    """assign_frames_wide with the populations of the queries through calculate_populations_against_wide_pruned: the same
    dict, the same values.  (A function of its own: assign_frames_wide's parameter list is pinned.)
    pruned_neighbours=True: the nearest reference frames through nearest_reference_wide_pruned as well, as
    assign_frames(..., pruned_neighbours=True) does below 65 columns."""
    return _assign_frames(queries, reference, radius, ref_states, _check_pair_wide(queries, reference), calculate_populations_wide,
                          calculate_populations_against_wide_pruned,
                          nearest_reference_wide_pruned if pruned_neighbours else nearest_reference_wide)


# ---- ... and both pruned cross sweeps for rows of 257..1024 columns (include/dc_density.h) -----------
def calculate_populations_against_xwide_pruned(queries, reference, radii, i_from=0, i_to=None, out=None):
    """calculate_populations_against_wide_pruned for rows of 257..1024 columns
    (dc_hip_populations_cross_xwide_pruned_dev): the populations of calculate_populations_against_xwide and of
    variant="direct" bit for bit, without the block pairs that cannot hold a pair within the radii.  In a cached workspace
    of its own kind (xwide_against_pruned_info reads its counters, xwide_against_pruned_order its two orders).  Other
    column counts raise."""
    sizes = _check_pair_xwide(queries, reference)
    out = _populations_against("dc_hip_populations_cross_xwide_pruned_dev", "xwide_against_pruned", queries, reference, sizes,
                               radii, i_from, i_to, out)
    _record_against_pruned(queries, sizes, i_from, i_to, "xwide_against_pruned")
    return out


def nearest_reference_xwide_pruned(queries, reference, fe_query=None, fe_ref=None, i_from=0, i_to=None):
    """nearest_reference_wide_pruned for rows of 257..1024 columns (dc_hip_nearest_neighbors_cross_xwide_pruned_dev): the
    four arrays of nearest_reference_xwide bit for bit; without free energies hd_idx / hd_d2 are None.  In the cached
    workspace of calculate_populations_against_xwide_pruned."""
    sizes = _check_pair_xwide(queries, reference)
    out = _nearest("dc_hip_nearest_neighbors_cross_xwide_pruned_dev", "xwide_against_pruned", queries, reference, sizes, fe_query,
                   fe_ref, i_from, i_to)
    _record_against_pruned(queries, sizes, i_from, i_to, "xwide_against_pruned")
    return out


def xwide_against_pruned_info(device):
    """(tiles, mfmas, exact_pairs) of the last pruned cross sweep of 257..1024 columns on this device, as
    wide_against_pruned_info gives them: the EVALUATED tile pairs (the neighbour call: summed over its launches);
    (0, 0, 0) when the direct kernel answered (flagged data), nothing was swept, or no such sweep has run."""
    return _wide_info("xwide_against_pruned", device)


def xwide_against_pruned_order(device):
    """both spatial orders of the last pruned cross sweep of 257..1024 columns on this device, position -> row, as
    wide_against_pruned_order gives them (dc_hip_cross_xwide_pruned_order_dev)."""
    return _against_pruned_order("xwide_against_pruned", "dc_hip_cross_xwide_pruned_order_dev", device)


def assign_frames_xwide_pruned(queries, reference, radius, ref_states, pruned_neighbours=False):
    """assign_frames_xwide on the pruned sweeps: the reference's own populations through
    calculate_populations_xwide_pruned, the queries' through calculate_populations_against_xwide_pruned; the same dict,
    the same values.  pruned_neighbours=True: the nearest reference frames through nearest_reference_xwide_pruned as well."""
    return _assign_frames(queries, reference, radius, ref_states, _check_pair_xwide(queries, reference),
                          calculate_populations_xwide_pruned, calculate_populations_against_xwide_pruned,
                          nearest_reference_xwide_pruned if pruned_neighbours else nearest_reference_xwide)


class Reference:
    """A resident reference for the pruned wide cross sweeps (dc_hip_reference_wide_*, 65..256 columns): the reference
    is prepared once, here; every batch of at most ``max_batch`` queries then pays for itself alone.

        with Reference(reference, max_batch=20000, radius=r, ref_states=states) as ref:
            for batch in batches:
                out = ref.assign(batch)            # the dict of assign_frames_wide_pruned, the same values

    or step by step: stage(queries), then populations(radii) and nearest(fe_query) in any order, any number of times.
    The results are those of calculate_populations_against_wide / nearest_reference_wide bit for bit.  The object keeps
    the reference tensor and the staged batch alive and allocates its workspace through torch on the reference's device.
    With ``radius`` and ``ref_states`` the construction runs calculate_populations_wide_pruned on the reference ONCE and keeps
    pops_ref, max_pop and fe_ref (set as the reference's free energies): what assign() needs of the reference."""

    _api = "dc_hip_reference_wide_"   # the entry points' common prefix
    _assign_open = "dc_hip_assign_open_wide_dev"   # ... and the assigner's open for this kind of handle
    _assign_h = _assign_ws = None     # the assigner of assign_device(), built on first use
    _cols = (65, 256, "the wide matrix-core sweeps take 65..256 columns")   # the widths of this kind, and its refusal

    def __init__(self, reference, max_batch, radius=None, ref_states=None):
        self._init(reference, max_batch, radius, ref_states)

    def _open_args(self, radius, max_radius):
        """what this kind's open call takes between max_batch and the workspace"""
        return ()

    def _self_populations(self, reference, radius):
        return calculate_populations_wide_pruned(reference, [radius])

    def _init(self, reference, max_batch, radius, ref_states, max_radius=None):
        """the construction of either kind: _cols, _open_args and _self_populations are what a kind supplies"""
        self._h = None
        self._n_ref, self._n_cols = _check_coords(reference)
        if not self._cols[0] <= self._n_cols <= self._cols[1]:
            raise ValueError(f"n_cols={self._n_cols}: {self._cols[2]}")
        self._max_batch = int(max_batch)
        if self._n_ref < 1 or self._max_batch < 1:
            raise ValueError(f"a reference of {self._n_ref} rows, batches of {self._max_batch}: both must be positive")
        if (radius is None) != (ref_states is None):
            raise ValueError("radius and ref_states go together")
        open_args = self._open_args(radius, max_radius)
        states = None if ref_states is None else np.ascontiguousarray(ref_states, dtype=np.int32)
        if states is not None and states.shape != (self._n_ref,):
            raise ValueError(f"ref_states must hold one state per reference row ({self._n_ref}), got shape {states.shape}")
        self._ref, self._queries, self._fe_ref = reference, None, None
        self.device = reference.device
        need = int(getattr(capi.lib, self._api + "workspace_bytes")(self._n_ref, self._n_cols, self._max_batch))
        self._ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            capi.check(getattr(capi.lib, self._api + "open_dev")(_dev(reference), self._n_ref, self._n_cols, self._max_batch,
                                                                 *open_args, _dev(self._ws), need, _stream_ptr(), C.byref(h)),
                       self._api + "open_dev")
        self._h = h
        self.radius, self.pops_ref, self.max_pop, self.fe_ref, self._states_r = radius, None, None, None, None
        if radius is not None:
            self._states_r = torch.as_tensor(states, device=self.device)
            self.pops_ref = self._self_populations(reference, radius)[0].contiguous()
            self.max_pop = int(self.pops_ref.max().item())
            self.fe_ref = calculate_free_energies(self.pops_ref)
            self.set_free_energies(self.fe_ref)

    n_ref = property(lambda self: self._n_ref)
    n_cols = property(lambda self: self._n_cols)
    max_batch = property(lambda self: self._max_batch)

    def close(self):
        if self._assign_h is not None:
            capi.lib.dc_hip_assign_close(self._assign_h)
            self._assign_h = None
        if self._h is not None:
            getattr(capi.lib, self._api + "close")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def _call(self, fn, *args):
        if self._h is None:
            raise ValueError("the reference is closed")
        with torch.cuda.device(self.device):
            capi.check(getattr(capi.lib, self._api + fn)(self._h, *args, _stream_ptr()), self._api + fn)

    def set_free_energies(self, fe_ref):
        """fe_ref: float32 CUDA [n_ref]; read by this call (the library keeps a copy in its workspace)"""
        assert fe_ref.is_cuda and fe_ref.dtype == torch.float32 and fe_ref.shape == (self._n_ref,) and fe_ref.is_contiguous()
        self._call("set_free_energies_dev", _dev(fe_ref))
        self._fe_ref = fe_ref

    def stage(self, queries):
        """the batch every sweep until the next stage() speaks of: float32 CUDA [n_q <= max_batch, n_cols]"""
        n_q, n_cols = _check_coords(queries)
        if n_cols != self._n_cols or queries.device != self.device:
            raise ValueError("queries and reference need the same n_cols and the same device")
        self._call("stage_dev", _dev(queries), n_q)
        self._queries = queries

    def populations(self, radii):
        """-> int32 [n_radii, n_q] of the staged batch, in the order of ``radii``"""
        if self._queries is None:
            raise ValueError("no batch is staged")
        rad = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        out = torch.empty((rad.size, self._queries.shape[0]), dtype=torch.int32, device=self.device)
        self._call("populations_dev", rad.ctypes.data_as(C.POINTER(C.c_float)), rad.size, _dev(out))
        return out

    def nearest(self, fe_query=None):
        """-> (nn_idx int32, nn_d2 float32, hd_idx, hd_d2) of the staged batch; without fe_query hd_idx / hd_d2 are None"""
        if self._queries is None:
            raise ValueError("no batch is staged")
        n_q, with_fe = self._queries.shape[0], fe_query is not None
        if with_fe:
            assert fe_query.is_cuda and fe_query.dtype == torch.float32 and fe_query.shape == (n_q,) and fe_query.is_contiguous()
        nn_idx = torch.empty(n_q, dtype=torch.int32, device=self.device)
        nn_d2 = torch.empty(n_q, dtype=torch.float32, device=self.device)
        hd_idx = torch.empty(n_q, dtype=torch.int32, device=self.device) if with_fe else None
        hd_d2 = torch.empty(n_q, dtype=torch.float32, device=self.device) if with_fe else None
        self._call("nearest_dev", _dev(fe_query) if with_fe else None, _dev(nn_idx), _dev(nn_d2),
                   _dev(hd_idx) if with_fe else None, _dev(hd_d2) if with_fe else None)
        return nn_idx, nn_d2, hd_idx, hd_d2

    def info(self):
        """(tiles, mfmas, exact_pairs, answered, reference_preparations) of the last sweep (dc_hip_reference_wide_info_dev)"""
        t, m, e, a, r = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        self._call("info_dev", C.byref(t), C.byref(m), C.byref(e), C.byref(a), C.byref(r))
        return int(t.value), int(m.value), int(e.value), int(a.value), int(r.value)

    def order(self):
        """(perm_q int32 [n_q of the staged batch] or None before a stage, perm_r int32 [n_ref]), position -> row"""
        perm_q = None if self._queries is None else torch.empty(self._queries.shape[0], dtype=torch.int32, device=self.device)
        perm_r = torch.empty(self._n_ref, dtype=torch.int32, device=self.device)
        self._call("order_dev", None if perm_q is None else _dev(perm_q), _dev(perm_r))
        return perm_q, perm_r

    def assign(self, queries):
        """assign_frames_wide_pruned(queries, reference, radius, ref_states, pruned_neighbours=True) without its work on
        the reference: any number of rows, in chunks of max_batch.  -> the same dict, the same values."""
        if self.radius is None:
            raise ValueError("assign() needs the radius and ref_states given at construction")
        n_q, _ = _check_coords(queries)
        none, parts = self._n_ref + 1, []
        for lo in range(0, max(n_q, 1), self._max_batch):
            chunk = queries[lo:lo + self._max_batch]
            self.stage(chunk)
            pops = self.populations([self.radius])[0].contiguous()
            fe = calculate_free_energies_against(pops, self.max_pop) if self.max_pop else \
                torch.full((chunk.shape[0],), float("inf"), dtype=torch.float32, device=self.device)
            nn_idx, nn_d2, hd_idx, hd_d2 = self.nearest(fe)
            states = torch.zeros(chunk.shape[0], dtype=torch.int32, device=self.device)
            pick = torch.where(hd_idx != none, hd_idx, nn_idx)
            ok = pick != none
            states[ok] = self._states_r[pick[ok].long()]
            parts.append({"states": states, "pops": pops, "fe": fe, "nn_idx": nn_idx, "nn_d2": nn_d2, "hd_idx": hd_idx, "hd_d2": hd_d2})
        out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
        out.update(pops_ref=self.pops_ref, max_pop=self.max_pop, fe_ref=self.fe_ref)
        return out


    def _assigner(self):
        """the dc_assign of this handle (dc_hip_assign_open[_wide]_dev), from radius, ref_states and max_pop; built once"""
        if self.radius is None:
            raise ValueError("assign_device() needs the radius and ref_states given at construction")
        if self._h is None:
            raise ValueError("the reference is closed")
        if self._assign_h is None:
            need = int(capi.lib.dc_hip_assign_workspace_bytes(self._n_ref, self._max_batch))
            self._assign_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
            h = C.c_void_p()
            with torch.cuda.device(self.device):
                capi.check(getattr(capi.lib, self._assign_open)(self._h, _dev(self._states_r), int(self.max_pop), float(self.radius),
                                                                _dev(self._assign_ws), need, _stream_ptr(), C.byref(h)),
                           self._assign_open)
            self._assign_h = h
        return self._assign_h

    def assign_device(self, queries):
        """assign() in one library call per chunk of max_batch rows (dc_hip_assign_batch_dev): the same dict, the same
        values, and no host synchronisation anywhere -- the free energies come from a table filled when the assigner is
        built (on the first call), the state pick is a kernel.  The call returns with its work queued on the current
        stream; the batch can be queued behind the one before it."""
        n_q, n_cols = _check_coords(queries)
        if n_cols != self._n_cols or queries.device != self.device:
            raise ValueError("queries and reference need the same n_cols and the same device")
        a = self._assigner()
        i32 = dict(dtype=torch.int32, device=self.device)
        f32 = dict(dtype=torch.float32, device=self.device)
        out = {"states": torch.empty(n_q, **i32), "pops": torch.empty(n_q, **i32), "fe": torch.empty(n_q, **f32),
               "nn_idx": torch.empty(n_q, **i32), "nn_d2": torch.empty(n_q, **f32), "hd_idx": torch.empty(n_q, **i32),
               "hd_d2": torch.empty(n_q, **f32)}
        with torch.cuda.device(self.device):
            stream = _stream_ptr()
            for lo in range(0, n_q, self._max_batch):
                n = min(self._max_batch, n_q - lo)
                capi.check(capi.lib.dc_hip_assign_batch_dev(a, C.c_void_p(queries.data_ptr() + 4 * lo * n_cols), n,
                                                            *(C.c_void_p(t.data_ptr() + 4 * lo) for t in out.values()), stream),
                           "dc_hip_assign_batch_dev")
                self._queries = queries[lo:lo + n]   # (what the handle has staged now)
        out.update(pops_ref=self.pops_ref, max_pop=self.max_pop, fe_ref=self.fe_ref)
        return out


class NarrowReference(Reference):
    """A resident reference for the pruned cross sweeps of rows of 1..64 columns (dc_hip_reference_*): Reference's
    methods, for calculate_populations_against(variant="cross_pruned") and nearest_reference(pruned=True).

        with NarrowReference(reference, max_batch=100000, radius=r, ref_states=states) as ref:
            for batch in batches:
                out = ref.assign(batch)   # the dict of assign_frames(variant="cross_pruned", pruned_neighbours=True)

    ``max_radius`` (default: ``radius``) is the largest radius any populations() call will use: the reference's operand
    image is built at the scale of that radius, and a larger one is refused.  With ``radius`` and ``ref_states`` the
    construction runs calculate_populations_partial (variant "auto") on the reference ONCE and keeps pops_ref, max_pop
    and fe_ref (set as the reference's free energies).  info() -> (tiles, mfmas, shares, answered,
    reference_preparations); order(which): 0 the population sweep's orders, 1 the neighbour sweep's."""
    _api = "dc_hip_reference_"
    _assign_open = "dc_hip_assign_open_dev"
    _cols = (1, 64, "the resident reference of the pruned cross sweeps takes 1..64 columns")

    def __init__(self, reference, max_batch, max_radius=None, radius=None, ref_states=None):
        self._init(reference, max_batch, radius, ref_states, max_radius)

    def _open_args(self, radius, max_radius):
        max_radius = radius if max_radius is None else max_radius
        if max_radius is None:
            raise ValueError("max_radius (or radius) is needed: the population scale is fixed when the reference is opened")
        self.max_radius = float(max_radius)
        return (self.max_radius,)

    def _self_populations(self, reference, radius):
        return calculate_populations_partial(reference, [radius], variant="auto")

    def info(self):
        """(tiles, mfmas, shares, answered, reference_preparations) of the last sweep (dc_hip_reference_info_dev)"""
        t, m, n, a, r = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        self._call("info_dev", C.byref(t), C.byref(m), C.byref(n), C.byref(a), C.byref(r))
        return int(t.value), int(m.value), int(n.value), int(a.value), int(r.value)

    def order(self, which=0):
        """(perm_q int32 [n_q of the staged batch] or None before a stage, perm_r int32 [n_ref]), position -> row, of the
        population sweep (which = 0) or of the neighbour sweep (which = 1)"""
        perm_q = None if self._queries is None else torch.empty(self._queries.shape[0], dtype=torch.int32, device=self.device)
        perm_r = torch.empty(self._n_ref, dtype=torch.int32, device=self.device)
        self._call("order_dev", int(which), None if perm_q is None else _dev(perm_q), _dev(perm_r))
        return perm_q, perm_r


class XWideReference(Reference):
    """A resident reference for the pruned cross sweeps of rows of 257..1024 columns (dc_hip_reference_xwide_*): Reference's
    methods, for calculate_populations_against_xwide_pruned and nearest_reference_xwide_pruned.

        with XWideReference(reference, max_batch=20000, radius=r, ref_states=states) as ref:
            for batch in batches:
                out = ref.assign(batch)   # the dict of assign_frames_xwide_pruned, the same values

    With ``radius`` and ``ref_states`` the construction runs calculate_populations_xwide_pruned on the reference ONCE."""
    _api = "dc_hip_reference_xwide_"
    _assign_open = "dc_hip_assign_open_xwide_dev"
    _cols = (257, 1024, "the extra-wide matrix-core sweeps take 257..1024 columns")

    def _self_populations(self, reference, radius):
        return calculate_populations_xwide_pruned(reference, [radius])


class Assigner:
    """The host-pointer assigner (dc_hip_assigner_*): what `clustering assign` and a C / C++ host run.  The library owns
    the device memory: it uploads ``reference_host`` [n_ref, n_cols] and ``ref_states`` [n_ref], runs the reference's
    self sweep at ``radius`` once, and opens the resident reference of the width.

        with Assigner(reference_host, ref_states, radius, max_batch=100000) as a:
            out = a.assign(queries_host)      # dict of numpy arrays: the values of assign_frames[_wide_pruned]

    ``path``: 0 the narrow handle (1..64 columns), 1 the wide handle (65..256), 2 the per-call cross entry points (any
    other width, or a reference the narrow handle refuses as too large), 3 the resident reference of 257..1024 columns
    (``xwide=True``, or DC_ASSIGN_XWIDE=1 in the environment; the same values as path 2)."""

    def __init__(self, reference_host, ref_states, radius, max_batch, device=0, xwide=False):
        self._h = None
        ref = np.ascontiguousarray(reference_host, dtype=np.float32)
        states = np.ascontiguousarray(ref_states, dtype=np.int32)
        if ref.ndim != 2 or states.shape != (ref.shape[0],):
            raise ValueError("reference_host must be [n_ref, n_cols] and ref_states hold one state per reference row")
        self.n_ref, self.n_cols = ref.shape
        h = C.c_void_p()
        args = (ref.ctypes.data_as(C.c_void_p), self.n_ref, self.n_cols, states.ctypes.data_as(C.c_void_p), float(radius),
                int(max_batch), int(device))
        if xwide:
            capi.check(capi.lib.dc_hip_assigner_open_flags(*args, capi.ASSIGNER_XWIDE_REFERENCE, C.byref(h)),
                       "dc_hip_assigner_open_flags")
        else:
            capi.check(capi.lib.dc_hip_assigner_open(*args, C.byref(h)), "dc_hip_assigner_open")
        self._h = h

    def close(self):
        if self._h is not None:
            capi.lib.dc_hip_assigner_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    @property
    def path(self):
        return int(capi.lib.dc_hip_assigner_path(self._h))

    def reference(self):
        """(pops_ref uint32 [n_ref], fe_ref float32 [n_ref], max_pop) of the reference's self sweep"""
        pops, fe, top = np.empty(self.n_ref, np.uint32), np.empty(self.n_ref, np.float32), C.c_uint32(0)
        capi.check(capi.lib.dc_hip_assigner_reference(self._h, pops.ctypes.data_as(C.c_void_p), fe.ctypes.data_as(C.c_void_p),
                                                      C.byref(top)), "dc_hip_assigner_reference")
        return pops, fe, int(top.value)

    def assign(self, queries_host):
        """-> dict of numpy arrays [n_q]: states int32, pops uint32, fe float32, nn_idx uint32, nn_d2 float32, hd_idx
        uint32, hd_d2 float32; any number of rows"""
        if self._h is None:
            raise ValueError("the assigner is closed")
        q = np.ascontiguousarray(queries_host, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.n_cols:
            raise ValueError("queries and reference need the same n_cols")
        n_q = q.shape[0]
        out = {"states": np.empty(n_q, np.int32), "pops": np.empty(n_q, np.uint32), "fe": np.empty(n_q, np.float32),
               "nn_idx": np.empty(n_q, np.uint32), "nn_d2": np.empty(n_q, np.float32), "hd_idx": np.empty(n_q, np.uint32),
               "hd_d2": np.empty(n_q, np.float32)}
        capi.check(capi.lib.dc_hip_assigner_assign(self._h, q.ctypes.data_as(C.c_void_p), n_q,
                                                   *(v.ctypes.data_as(C.c_void_p) for v in out.values())),
                   "dc_hip_assigner_assign")
        return out


def evaluated_tiles(device):
    """(pop_tiles, nn_tiles): 32x32 frame-pair tiles evaluated by the last pruned sweeps on this device's
    workspace.  The header is rebuilt by every sweep, so read it right after the sweep of interest
    (the other counter is then 0)."""
    ws = _workspace(device)
    if ws.buf is None:
        return 0, 0
    a, b = C.c_uint64(0), C.c_uint64(0)
    with torch.cuda.device(device):
        rc = capi.lib.dc_hip_workspace_counters_dev(_dev(ws.buf), C.byref(a), C.byref(b), _stream_ptr())
    capi.check(rc, "dc_hip_workspace_counters_dev")
    return int(a.value), int(b.value)


def evaluated_tiles_against(device):
    """(pop_tiles, pop_mfma): 32x32 frame-pair tiles evaluated and MFMA instructions issued by the last
    calculate_populations_against(..., variant="cross_pruned") on this device (all radii of the call together); the
    counters of its workspace, read like evaluated_tiles.  (0, 0) after a call the pruned sweep did not answer."""
    ws = _cross_pruned_workspace(device)
    if ws.buf is None:
        return 0, 0
    a, b, m, n = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    with torch.cuda.device(device):
        capi.check(capi.lib.dc_hip_workspace_counters_dev(_dev(ws.buf), C.byref(a), C.byref(b), _stream_ptr()),
                   "dc_hip_workspace_counters_dev")
        capi.check(capi.lib.dc_hip_workspace_mfma_counters_dev(_dev(ws.buf), C.byref(m), C.byref(n), _stream_ptr()),
                   "dc_hip_workspace_mfma_counters_dev")
    return int(a.value), int(m.value)


def issued_mfmas(device):
    """(pop, nn): v_mfma_f32_32x32x16_f16 instructions the last pruned sweeps on this device's workspace issued, counted by
    the kernels (dc_hip_workspace_mfma_counters_dev); read right after the sweep of interest, like evaluated_tiles"""
    ws = _workspace(device)
    if ws.buf is None:
        return 0, 0
    a, b = C.c_uint64(0), C.c_uint64(0)
    with torch.cuda.device(device):
        capi.check(capi.lib.dc_hip_workspace_mfma_counters_dev(_dev(ws.buf), C.byref(a), C.byref(b), _stream_ptr()),
                   "dc_hip_workspace_mfma_counters_dev")
    return int(a.value), int(b.value)


def components_info(coords):
    """of the last pruned population sweep over coords on its device: dict(n_components, extent2_global, extent2_local,
    scale) -- dc_hip_workspace_components_dev"""
    n_rows, n_cols = _check_coords(coords)
    ws = _workspace(coords.device)
    n, a, b, s = C.c_uint32(0), C.c_float(0), C.c_float(0), C.c_float(0)
    with torch.cuda.device(coords.device):
        capi.check(capi.lib.dc_hip_workspace_components_dev(_dev(ws.buf), n_rows, n_cols, C.byref(n), C.byref(a),
                                                            C.byref(b), C.byref(s), _stream_ptr()),
                   "dc_hip_workspace_components_dev")
    return {"n_components": int(n.value), "extent2_global": float(a.value), "extent2_local": float(b.value),
            "scale": float(s.value)}


def sweep_timing(enable):
    """dc_hip_sweep_timing: bracket the main sweep kernels with HIP events (measurement aid of bench.py)"""
    capi.check(capi.lib.dc_hip_sweep_timing(1 if enable else 0), "dc_hip_sweep_timing")


def last_sweep_ms(kind, device):
    """duration in ms of the main sweep kernel(s) of one kind ("pop" / "nn") since the last read (synchronises)"""
    ms = C.c_float(0.0)
    with torch.cuda.device(device):
        capi.check(capi.lib.dc_hip_last_sweep_ms(0 if kind == "pop" else 1, C.byref(ms)), "dc_hip_last_sweep_ms")
    return float(ms.value)


def radius_pairs(coords, r2, capacity=None):
    """All unordered frame pairs with canonical d2 < r2 (the radius graph of the reference's screening,
    density_clustering.cpp:292-332) -> (pairs int64 [n_pairs, 2] on the device, pops int32 [n_rows]).
    One counting sweep sizes the buffer unless a capacity is given.  Any n_cols; rows with inf / NaN
    have no partners (population 1), like in the reference."""
    n_rows, n_cols = _check_coords(coords)
    dev = coords.device
    pops = torch.empty(n_rows, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def sweep(pairs, cap):
        with torch.cuda.device(dev):
            ws, ws_bytes = _workspace(dev).get(n_rows, n_cols, 1)
            rc = capi.lib.dc_hip_radius_pairs_dev(_dev(coords), n_rows, n_cols, float(r2), _dev(pops),
                                                  _dev(pairs) if pairs is not None else None, cap,
                                                  _dev(count), ws, ws_bytes, _stream_ptr())
        capi.check(rc, "dc_hip_radius_pairs_dev")
        return int(count.item())

    if capacity is None:
        capacity = sweep(None, 0)
    pairs = torch.empty((max(capacity, 1), 2), dtype=torch.int32, device=dev)
    n = sweep(pairs, capacity)
    if n > capacity:
        return radius_pairs(coords, r2, n)
    return pairs[:n].to(torch.int64), pops


def radius_min_edge(coords, r2, comp, rank, segment=0, n_segments=0):
    """One Boruvka round on the radius graph (dc_hip_radius_min_edge[_segment]_dev): comp, rank int32
    CUDA [n_rows] -> (best int64 [n_rows]: (max rank << 32 | min rank) of the lightest pair leaving
    component id, -1 (all ones) if none; pops int32 [n_rows]).  n_segments > 0: what the queries of one
    segment of a sharded run see (partials merge by unsigned minimum / summation).  Any n_cols and
    non-finite coordinates, like radius_pairs."""
    n_rows, n_cols = _check_coords(coords)
    dev = coords.device
    for t in (comp, rank):
        assert t.is_cuda and t.dtype == torch.int32 and t.shape == (n_rows,) and t.is_contiguous()
    best = torch.empty(n_rows, dtype=torch.int64, device=dev)
    pops = torch.empty(n_rows, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, ws_bytes = _workspace(dev).get(n_rows, n_cols, 1)
        rc = capi.lib.dc_hip_radius_min_edge_segment_dev(_dev(coords), n_rows, n_cols, float(r2), _dev(comp),
                                                         _dev(rank), segment, n_segments, _dev(best),
                                                         _dev(pops), ws, ws_bytes, _stream_ptr())
    capi.check(rc, "dc_hip_radius_min_edge_segment_dev")
    return best, pops


def radius_forest(coords_host, r2, rank, device=0):
    """Bottleneck spanning forest of the radius graph (dc_hip_radius_forest).  coords_host: float32
    numpy [n_rows, n_cols]; rank: permutation of 0..n_rows-1 -> (edges uint32 numpy [n_edges, 2] of
    frame ids, number of sweeps).  Any n_cols and non-finite coordinates, like radius_pairs."""
    coords_host = np.ascontiguousarray(coords_host, dtype=np.float32)
    n_rows, n_cols = coords_host.shape
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    assert rank.shape == (n_rows,)
    edges = np.empty((max(n_rows - 1, 1), 2), dtype=np.uint32)
    n_edges, n_rounds = C.c_size_t(0), C.c_uint32(0)
    rc = capi.lib.dc_hip_radius_forest(coords_host.ctypes.data_as(C.c_void_p), n_rows, n_cols, float(r2),
                                       rank.ctypes.data_as(C.c_void_p), device,
                                       edges.ctypes.data_as(C.c_void_p), C.byref(n_edges),
                                       C.byref(n_rounds))
    capi.check(rc, "dc_hip_radius_forest")
    return edges[:n_edges.value].copy(), int(n_rounds.value)


# ---- the radius graph on the wide matrix-core sweep (65..256 columns; include/dc_density.h) -------------------------
_WIDE_COLS, _XWIDE_COLS = (65, 256), (257, 1024)   # the widths of the two families of wide matrix-core sweeps


def _check_coords_wide(coords, cols=_WIDE_COLS):
    """_check_coords, the column count (refused here as the library refuses it: 65..256, or the ``cols`` of the family) first"""
    if isinstance(coords, (torch.Tensor, np.ndarray)) and coords.ndim == 2 and not cols[0] <= coords.shape[1] <= cols[1]:
        raise ValueError(f"n_cols={coords.shape[1]}: the wide matrix-core sweeps take {cols[0]}..{cols[1]} columns")
    return _check_coords(coords) if isinstance(coords, torch.Tensor) else coords.shape


def radius_pairs_wide(coords, r2, capacity=None):
    """radius_pairs for rows of 65..256 columns on the matrix cores (dc_hip_radius_pairs_wide_dev): all unordered frame
    pairs with canonical d2 < r2 -> (pairs int64 [n_pairs, 2] on the device, pops int32 [n_rows]).  One counting sweep
    sizes the buffer unless a capacity is given.  Rows with inf / NaN have no partners (population 1; the direct kernel
    answers such data).  In the cached workspace of the wide sweeps (wide_sweep_info reads its counters).  Other column
    counts raise."""
    return _radius_pairs_wide("dc_hip_radius_pairs_wide_dev", "wide", coords, r2, capacity)


def _radius_pairs_wide(fn, kind, coords, r2, capacity, cols=_WIDE_COLS):
    n_rows, n_cols = _check_coords_wide(coords, cols)
    dev = coords.device
    pops = torch.empty(n_rows, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)

    def sweep(pairs, cap):
        with torch.cuda.device(dev):
            ws, ws_bytes = _get(kind, dev, n_rows, n_cols, 1)
            rc = getattr(capi.lib, fn)(_dev(coords), n_rows, n_cols, float(r2), _dev(pops),
                                       _dev(pairs) if pairs is not None else None, cap,
                                       _dev(count), ws, ws_bytes, _stream_ptr())
        capi.check(rc, fn)
        return int(count.item())

    if capacity is None:
        capacity = sweep(None, 0)
    pairs = torch.empty((max(capacity, 1), 2), dtype=torch.int32, device=dev)
    n = sweep(pairs, capacity)
    if n > capacity:
        return _radius_pairs_wide(fn, kind, coords, r2, n, cols)
    return pairs[:n].to(torch.int64), pops


def radius_min_edge_wide(coords, r2, comp, rank, segment=0, n_segments=0):
    """radius_min_edge for rows of 65..256 columns on the matrix cores (dc_hip_radius_min_edge_wide_dev): comp, rank
    int32 CUDA [n_rows] -> (best int64 [n_rows]: (max rank << 32 | min rank) of the lightest pair leaving component
    id, -1 (all ones) if none; pops int32 [n_rows]).  n_segments > 0: what the queries of one row block of a sharded
    run see (partials merge by unsigned minimum / summation), array-equal to radius_min_edge of that segment.  Other
    column counts raise."""
    return _radius_min_edge_wide("dc_hip_radius_min_edge_wide_dev", "wide", coords, r2, comp, rank, segment, n_segments)


def _radius_min_edge_wide(fn, kind, coords, r2, comp, rank, segment, n_segments, cols=_WIDE_COLS):
    n_rows, n_cols = _check_coords_wide(coords, cols)
    dev = coords.device
    for t in (comp, rank):
        assert t.is_cuda and t.dtype == torch.int32 and t.shape == (n_rows,) and t.is_contiguous()
    best = torch.empty(n_rows, dtype=torch.int64, device=dev)
    pops = torch.empty(n_rows, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, ws_bytes = _get(kind, dev, n_rows, n_cols, 1)
        rc = getattr(capi.lib, fn)(_dev(coords), n_rows, n_cols, float(r2), _dev(comp), _dev(rank), segment, n_segments,
                                   _dev(best), _dev(pops), ws, ws_bytes, _stream_ptr())
    capi.check(rc, fn)
    return best, pops


def radius_forest_wide(coords_host, r2, rank, device=0):
    """radius_forest for rows of 65..256 columns on the matrix cores (dc_hip_radius_forest_wide; one device, no
    session).  coords_host: float32 numpy [n_rows, n_cols]; rank: permutation of 0..n_rows-1 -> (edges uint32 numpy
    [n_edges, 2] of frame ids, number of sweeps).  Other column counts raise."""
    return _radius_forest_wide("dc_hip_radius_forest_wide", coords_host, r2, rank, device)


def _radius_forest_wide(fn, coords_host, r2, rank, device, cols=_WIDE_COLS):
    coords_host = np.ascontiguousarray(coords_host, dtype=np.float32)
    n_rows, n_cols = _check_coords_wide(coords_host, cols)
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    assert rank.shape == (n_rows,)
    edges = np.empty((max(n_rows - 1, 1), 2), dtype=np.uint32)
    n_edges, n_rounds = C.c_size_t(0), C.c_uint32(0)
    rc = getattr(capi.lib, fn)(coords_host.ctypes.data_as(C.c_void_p), n_rows, n_cols, float(r2),
                               rank.ctypes.data_as(C.c_void_p), device,
                               edges.ctypes.data_as(C.c_void_p), C.byref(n_edges), C.byref(n_rounds))
    capi.check(rc, fn)
    return edges[:n_edges.value].copy(), int(n_rounds.value)


# ---- ... and its pruned form (include/dc_density.h, the PRUNED radius graph) -----------------------------------------
def radius_pairs_wide_pruned(coords, r2, capacity=None):
    """radius_pairs_wide without the block pairs that cannot hold a pair within the radius
    (dc_hip_radius_pairs_wide_pruned_dev): the same set of pairs -- in no order within a pair -- and the same
    populations.  In the cached workspace of the pruned wide sweeps (wide_pruned_info reads its counters,
    wide_pruned_order its order)."""
    out = _radius_pairs_wide("dc_hip_radius_pairs_wide_pruned_dev", "wide_pruned", coords, r2, capacity)
    _shapes["wide_pruned"][str(coords.device)] = tuple(coords.shape)
    return out


def radius_min_edge_wide_pruned(coords, r2, comp, rank, segment=0, n_segments=0):
    """radius_min_edge_wide on the pruned sweep (dc_hip_radius_min_edge_wide_pruned_dev): the whole round (n_segments
    == 0) is array-equal to it; n_segments > 0: what the queries of the blocks segment, segment + n_segments, ... of
    the spatial order see (partials merge by unsigned minimum / summation; pops are non-zero only on the rows of those
    blocks).  wide_pruned_info and wide_pruned_order as above."""
    out = _radius_min_edge_wide("dc_hip_radius_min_edge_wide_pruned_dev", "wide_pruned", coords, r2, comp, rank,
                                segment, n_segments)
    _shapes["wide_pruned"][str(coords.device)] = tuple(coords.shape)
    return out


def radius_forest_wide_pruned(coords_host, r2, rank, device=0):
    """radius_forest_wide on the pruned sweep (dc_hip_radius_forest_wide_pruned): the same edges and rounds; the order
    is built once per forest."""
    return _radius_forest_wide("dc_hip_radius_forest_wide_pruned", coords_host, r2, rank, device)


# ---- ... and both forms at 257..1024 columns (include/dc_density.h, the radius graph at 257..1024 columns) -----------
def radius_pairs_xwide(coords, r2, capacity=None):
    """radius_pairs_wide for rows of 257..1024 columns (dc_hip_radius_pairs_xwide_dev): the same contract, in the cached
    workspace of the unpruned sweeps of those widths (xwide_sweep_info reads its counters).  Other column counts raise."""
    return _radius_pairs_wide("dc_hip_radius_pairs_xwide_dev", "xwide", coords, r2, capacity, _XWIDE_COLS)


def radius_min_edge_xwide(coords, r2, comp, rank, segment=0, n_segments=0):
    """radius_min_edge_wide for rows of 257..1024 columns (dc_hip_radius_min_edge_xwide_dev): a segment is the
    reference's row block.  Other column counts raise."""
    return _radius_min_edge_wide("dc_hip_radius_min_edge_xwide_dev", "xwide", coords, r2, comp, rank, segment, n_segments,
                                 _XWIDE_COLS)


def radius_forest_xwide(coords_host, r2, rank, device=0):
    """radius_forest_wide for rows of 257..1024 columns (dc_hip_radius_forest_xwide).  Other column counts raise."""
    return _radius_forest_wide("dc_hip_radius_forest_xwide", coords_host, r2, rank, device, _XWIDE_COLS)


def radius_pairs_xwide_pruned(coords, r2, capacity=None):
    """radius_pairs_wide_pruned for rows of 257..1024 columns (dc_hip_radius_pairs_xwide_pruned_dev): the set of pairs of
    radius_pairs_xwide -- in no order within a pair -- and the same populations.  In the cached workspace of the pruned
    sweeps of those widths (xwide_pruned_info reads its counters, xwide_pruned_order its order)."""
    out = _radius_pairs_wide("dc_hip_radius_pairs_xwide_pruned_dev", "xwide_pruned", coords, r2, capacity, _XWIDE_COLS)
    _shapes["xwide_pruned"][str(coords.device)] = tuple(coords.shape)
    return out


def radius_min_edge_xwide_pruned(coords, r2, comp, rank, segment=0, n_segments=0):
    """radius_min_edge_wide_pruned for rows of 257..1024 columns (dc_hip_radius_min_edge_xwide_pruned_dev): the whole
    round is array-equal to radius_min_edge_xwide; n_segments > 0: the query blocks segment, segment + n_segments, ... of
    the order (partials merge by unsigned minimum / summation)."""
    out = _radius_min_edge_wide("dc_hip_radius_min_edge_xwide_pruned_dev", "xwide_pruned", coords, r2, comp, rank,
                                segment, n_segments, _XWIDE_COLS)
    _shapes["xwide_pruned"][str(coords.device)] = tuple(coords.shape)
    return out


def radius_forest_xwide_pruned(coords_host, r2, rank, device=0):
    """radius_forest_xwide on the pruned sweep (dc_hip_radius_forest_xwide_pruned): the same edges and rounds; the order
    is built once per forest."""
    return _radius_forest_wide("dc_hip_radius_forest_xwide_pruned", coords_host, r2, rank, device, _XWIDE_COLS)


def pack_neighbors(nn_idx, nn_d2, hd_idx, hd_d2):
    """-> int64 CUDA [2, n_rows]: (d2 bits << 32 | index) words of nn and nn_hd (dc_hip_neighbors_pack_dev);
    partial results of a sharded run merge with all_reduce(min)."""
    n = nn_idx.shape[0]
    words = torch.empty((2, n), dtype=torch.int64, device=nn_idx.device)
    with torch.cuda.device(nn_idx.device):
        rc = capi.lib.dc_hip_neighbors_pack_dev(_dev(nn_idx), _dev(nn_d2), _dev(hd_idx), _dev(hd_d2), n,
                                                _dev(words), _stream_ptr())
    capi.check(rc, "dc_hip_neighbors_pack_dev")
    return words


def unpack_neighbors(words, out=None):
    """inverse of pack_neighbors -> (nn_idx int32, nn_d2 float32, hd_idx int32, hd_d2 float32)"""
    n = words.shape[1]
    dev = words.device
    if out is None:
        out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    with torch.cuda.device(dev):
        rc = capi.lib.dc_hip_neighbors_unpack_dev(_dev(words), n, _dev(out[0]), _dev(out[1]), _dev(out[2]),
                                                  _dev(out[3]), _stream_ptr())
    capi.check(rc, "dc_hip_neighbors_unpack_dev")
    return out


def neighbor_block_rows(n_rows, n_cols, n_segments):
    """rows of one rank's block in the all-gather merge of the neighbour partials (dc_hip_neighbors_block_rows)"""
    return int(capi.lib.dc_hip_neighbors_block_rows(n_rows, n_cols, n_segments))


def _pack_block(fn, kind, rows, coords, results, segment, n_segments, out, variant=None):
    """One block pack call of ``fn`` in the cached workspace of ``kind``; rows: the block's rows -> int32 [4, rows]"""
    n_rows, n_cols = _check_coords(coords)
    rows = rows(n_rows, n_cols, n_segments)
    if out is None:
        out = torch.empty((4, rows), dtype=torch.int32, device=coords.device)
    assert out.shape == (4, rows) and out.dtype == torch.int32 and out.is_contiguous()
    with torch.cuda.device(coords.device):
        ws, ws_bytes = _get(kind, coords.device, n_rows, n_cols, 1)
        rc = getattr(capi.lib, fn)(*[_dev(t) for t in results], n_rows, n_cols, segment, n_segments, ws, ws_bytes,
                                   *(() if variant is None else (variant,)), _dev(out), _stream_ptr())
    capi.check(rc, fn)
    return out


def _unpack_blocks(fn, kind, rows, coords, blocks, n_segments, out, check, variant=None, no_workspace=None):
    """One block unpack call of ``fn`` in the cached workspace of ``kind``; no_workspace: what check=True does first for a
    shape without one.  -> (the four arrays, bytes of the workspace)"""
    n_rows, n_cols = _check_coords(coords)
    dev = coords.device
    rows = rows(n_rows, n_cols, n_segments)
    assert blocks.is_contiguous() and blocks.dtype == torch.int32 and blocks.numel() == n_segments * 4 * rows
    if out is None:
        buf = (torch.empty if check else torch.zeros)((4, n_rows), dtype=torch.int32, device=dev)   # (one fill, not four)
        out = (buf[0], buf[1].view(torch.float32), buf[2], buf[3].view(torch.float32))
    with torch.cuda.device(dev):
        ws, ws_bytes = _get(kind, dev, n_rows, n_cols, 1)
        if check and not ws_bytes and no_workspace:
            no_workspace(blocks.view(n_segments, 4, rows))
        rc = getattr(capi.lib, fn)(_dev(blocks), n_rows, n_cols, n_segments, ws, ws_bytes, *(() if variant is None else (variant,)),
                                   _dev(out[0]), _dev(out[1]), _dev(out[2]), _dev(out[3]), _stream_ptr())
    capi.check(rc, fn)
    return out, ws_bytes


def _layout_status(fn, kind, device):
    """the verdict word of the last block unpack in this device's workspace of ``kind``, read by ``fn``; synchronises"""
    ws = _cached(kind, device)
    if ws.buf is None:
        return False
    bad = C.c_int(0)
    with torch.cuda.device(device):
        capi.check(getattr(capi.lib, fn)(_dev(ws.buf), C.byref(bad), _stream_ptr()), fn)
    return bool(bad.value)


def pack_neighbor_block(coords, nn_idx, nn_d2, hd_idx, hd_d2, segment, n_segments, variant="auto", out=None):
    """The results of this segment's own rows as a dense block int32 [4, block_rows] (dc_hip_neighbors_block_pack_dev);
    call right after nearest_neighbors_segment on the same device (its ordering is read from the workspace)."""
    return _pack_block("dc_hip_neighbors_block_pack_dev", "self", neighbor_block_rows, coords, (nn_idx, nn_d2, hd_idx, hd_d2),
                       segment, n_segments, out, capi.VARIANTS[variant])


BLOCK_HEADER_ROWS = 32    # the last entries of plane 0 of a block: its layout header (dc_mfma.hip nn_block_pack_kernel)


def check_neighbor_block_layout(blocks):
    """All ranks must have packed their blocks under the SAME layout (by position or row block, the same padded order,
    group size and deal -- words 0..6 of the header); a rank that derived another order would have its rows scattered
    to the wrong frames without any other sign.  One small device comparison + a synchronisation."""
    hdr = blocks[:, 0, -BLOCK_HEADER_ROWS:-BLOCK_HEADER_ROWS + 8]
    if not bool((hdr == hdr[0:1]).all()):
        raise RuntimeError("neighbour blocks of the ranks were packed under different layouts: " + str(hdr.cpu().tolist()))


def layout_status(device):
    """True if the last dc_hip_neighbors_block_unpack_dev in this device's workspace REFUSED its blocks (their layout headers
    differed: nothing was unpacked) -- dc_hip_workspace_layout_status_dev; synchronises"""
    return _layout_status("dc_hip_workspace_layout_status_dev", "self", device)


def unpack_neighbor_blocks(coords, blocks, n_segments, variant="auto", out=None, check=True):
    """blocks int32 [n_segments, 4, block_rows] gathered from all ranks -> (nn_idx, nn_d2, hd_idx, hd_d2) by frame
    (dc_hip_neighbors_block_unpack_dev).  The unpack kernel compares the blocks' layout headers itself and writes nothing
    on a mismatch; check=True asks for its verdict right away (one synchronisation) and raises.  check=False leaves that to
    the caller: layout_status() BEFORE the next call into the workspace -- the verdict word describes the last unpack only,
    the next unpack or sweep replaces it -- and on a mismatch the returned arrays hold whatever they held before (zeros
    here: a refused unpack must not hand out uninitialised memory as neighbours)."""
    # (no workspace for the kernel to flag in -- shapes without a matrix-core sweep: the headers are compared here)
    out, ws_bytes = _unpack_blocks("dc_hip_neighbors_block_unpack_dev", "self", neighbor_block_rows, coords, blocks, n_segments, out,
                                   check, capi.VARIANTS[variant], no_workspace=check_neighbor_block_layout)
    if check and ws_bytes and layout_status(coords.device):
        check_neighbor_block_layout(blocks.view(n_segments, 4, -1))   # (raises, with the headers in the message)
        raise RuntimeError("neighbour blocks of the ranks were packed under different layouts")
    return out


# ---- ... and the blocks of a sharded run of the pruned WIDE neighbour sweep (65..256 columns) ---------------------------
def neighbor_block_rows_wide(n_rows, n_cols, n_segments):
    """rows of one rank's block in the wide order (dc_hip_neighbors_block_rows_wide): the larger of the largest segment in
    positions and the largest row block, plus the 32 header entries"""
    return int(capi.lib.dc_hip_neighbors_block_rows_wide(n_rows, n_cols, n_segments))


def pack_neighbor_block_wide(coords, nn_idx, nn_d2, hd_idx, hd_d2, segment, n_segments, out=None):
    """The results of this segment's blocks of the order as a dense block int32 [4, block_rows]
    (dc_hip_neighbors_block_pack_wide_dev); call right after nearest_neighbors_wide_pruned(coords, fe, segment, n_segments)
    on the same device: the order and the flag of its data are read from the workspace of the pruned wide sweeps."""
    return _pack_block("dc_hip_neighbors_block_pack_wide_dev", "wide_pruned", neighbor_block_rows_wide, coords,
                       (nn_idx, nn_d2, hd_idx, hd_d2), segment, n_segments, out)


def wide_layout_status(device):
    """True if the last dc_hip_neighbors_block_unpack_wide_dev in this device's workspace of the pruned wide sweeps REFUSED
    its blocks (nothing was unpacked) -- dc_hip_wide_layout_status_dev; synchronises"""
    return _layout_status("dc_hip_wide_layout_status_dev", "wide_pruned", device)


def unpack_neighbor_blocks_wide(coords, blocks, n_segments, out=None, check=True):
    """blocks int32 [n_segments, 4, block_rows] gathered from all ranks -> (nn_idx, nn_d2, hd_idx, hd_d2) by frame
    (dc_hip_neighbors_block_unpack_wide_dev), in the workspace of the pruned wide sweeps of this device, which must hold
    the order the blocks were packed by.  The kernel compares the layout headers itself and writes nothing on a mismatch;
    check=True asks for its verdict right away (one synchronisation) and raises, check=False leaves that to the caller
    (wide_layout_status) -- the arrays handed out then hold what they held before (zeros if made here)."""
    out, _ = _unpack_blocks("dc_hip_neighbors_block_unpack_wide_dev", "wide_pruned", neighbor_block_rows_wide, coords, blocks,
                            n_segments, out, check)
    if check and coords.shape[0] and wide_layout_status(coords.device):
        raise RuntimeError("neighbour blocks of the ranks were packed under different layouts")
    return out


# ---- ... and of the pruned neighbour sweep of 257..1024 columns --------------------------------------------------------
def neighbor_block_rows_xwide(n_rows, n_cols, n_segments):
    """neighbor_block_rows_wide for 257..1024 columns (dc_hip_neighbors_block_rows_xwide); 0 outside them"""
    return int(capi.lib.dc_hip_neighbors_block_rows_xwide(n_rows, n_cols, n_segments))


def pack_neighbor_block_xwide(coords, nn_idx, nn_d2, hd_idx, hd_d2, segment, n_segments, out=None):
    """pack_neighbor_block_wide for 257..1024 columns (dc_hip_neighbors_block_pack_xwide_dev); call right after
    nearest_neighbors_xwide_pruned(coords, fe, segment, n_segments) on the same device."""
    return _pack_block("dc_hip_neighbors_block_pack_xwide_dev", "xwide_pruned", neighbor_block_rows_xwide, coords,
                       (nn_idx, nn_d2, hd_idx, hd_d2), segment, n_segments, out)


def xwide_layout_status(device):
    """True if the last dc_hip_neighbors_block_unpack_xwide_dev in this device's workspace of the pruned sweeps of 257..1024
    columns REFUSED its blocks (nothing was unpacked) -- dc_hip_xwide_layout_status_dev; synchronises"""
    return _layout_status("dc_hip_xwide_layout_status_dev", "xwide_pruned", device)


def unpack_neighbor_blocks_xwide(coords, blocks, n_segments, out=None, check=True):
    """unpack_neighbor_blocks_wide for 257..1024 columns (dc_hip_neighbors_block_unpack_xwide_dev), in the workspace of the
    pruned sweeps of those widths on this device, which must hold the order the blocks were packed by."""
    out, _ = _unpack_blocks("dc_hip_neighbors_block_unpack_xwide_dev", "xwide_pruned", neighbor_block_rows_xwide, coords, blocks,
                            n_segments, out, check)
    if check and coords.shape[0] and xwide_layout_status(coords.device):
        raise RuntimeError("neighbour blocks of the ranks were packed under different layouts")
    return out


def compute_sigma2(nn_d2):
    """compute_sigma2 (density_clustering.cpp:334-343)."""
    out = C.c_double(0.0)
    with torch.cuda.device(nn_d2.device):
        rc = capi.lib.dc_hip_sigma2_dev(_dev(nn_d2), nn_d2.shape[0], C.byref(out), _stream_ptr())
    capi.check(rc, "dc_hip_sigma2_dev")
    return out.value


class Session:
    """A trajectory resident on the GPUs of this process across pop -> FE -> NN -> forest
    (dc_hip_session_*, include/dc_density.h): HOST numpy arrays in and out, one upload per device, partial
    results of several devices merged on the devices over RCCL.  This is the path the C++ shim and the
    command line take; tests use it to compare the resident flow with the call-by-call one."""

    def __init__(self, coords_host, n_devices=0, devices=None, wide=False):
        """wide=True: dc_hip_session_open_flags(DC_SESSION_WIDE_SWEEPS) -- at 65..256 columns the pruned wide matrix-core
        sweeps answer; wide=False: dc_hip_session_open (which the environment's DC_SESSION_WIDE=1 turns into the same)"""
        c = np.ascontiguousarray(coords_host, dtype=np.float32)
        assert c.ndim == 2
        self.n_rows, self.n_cols = c.shape
        self._h = C.c_void_p(0)
        devs = None
        if devices is not None:
            devs = (C.c_int * len(devices))(*devices)
            n_devices = len(devices)
        if wide:
            capi.check(capi.lib.dc_hip_session_open_flags(c.ctypes.data_as(C.c_void_p), self.n_rows, self.n_cols, devs,
                                                          n_devices, capi.SESSION_WIDE_SWEEPS, C.byref(self._h)),
                       "dc_hip_session_open_flags")
        else:
            capi.check(capi.lib.dc_hip_session_open(c.ctypes.data_as(C.c_void_p), self.n_rows, self.n_cols, devs,
                                                    n_devices, C.byref(self._h)), "dc_hip_session_open")

    def close(self):
        if self._h:
            capi.lib.dc_hip_session_close(self._h)
            self._h = C.c_void_p(0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    @property
    def n_devices(self):
        return int(capi.lib.dc_hip_session_devices(self._h))

    @property
    def wide(self):
        """True if the session runs the pruned wide sweeps (the flag, and 65..256 columns): dc_hip_session_wide"""
        return bool(capi.lib.dc_hip_session_wide(self._h))

    @property
    def uses_rccl(self):
        return bool(capi.lib.dc_hip_session_uses_rccl(self._h))

    @property
    def merge_mode(self):
        """0: one device; 1: RCCL collectives on the devices; 2: through the host (the reference's own merge)"""
        return int(capi.lib.dc_hip_session_merge_mode(self._h))

    @property
    def merge_note(self):
        """dc_hip_session_merge_note: which merge runs and, for the host merge, why RCCL is not used"""
        return capi.lib.dc_hip_session_merge_note(self._h).decode("utf-8", "replace")

    def counters(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        capi.check(capi.lib.dc_hip_session_counters(self._h, C.byref(a), C.byref(b)), "dc_hip_session_counters")
        return int(a.value), int(b.value)

    def populations(self, radii, fetch=True):
        rad = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
        out = np.empty((rad.size, self.n_rows), dtype=np.uint32) if fetch else None
        capi.check(capi.lib.dc_hip_session_populations(self._h, rad.ctypes.data_as(C.c_void_p), rad.size,
                                                       out.ctypes.data_as(C.c_void_p) if fetch else None),
                   "dc_hip_session_populations")
        return out

    def free_energies(self, radius_index=0, fetch=True, max_pop=False):
        """-> fe float32 [n_rows] (None unless fetch); max_pop=True: (fe, the largest resident population of that radius)"""
        out = np.empty(self.n_rows, dtype=np.float32) if fetch else None
        mx = C.c_uint32(0)
        capi.check(capi.lib.dc_hip_session_free_energies(self._h, radius_index,
                                                         out.ctypes.data_as(C.c_void_p) if fetch else None,
                                                         C.byref(mx) if max_pop else None),
                   "dc_hip_session_free_energies")
        return (out, int(mx.value)) if max_pop else out

    def set_free_energies(self, fe):
        f = np.ascontiguousarray(fe, dtype=np.float32)
        assert f.shape == (self.n_rows,)
        capi.check(capi.lib.dc_hip_session_set_free_energies(self._h, f.ctypes.data_as(C.c_void_p)),
                   "dc_hip_session_set_free_energies")

    def nearest_neighbors(self, nn_idx=True, nn_d2=True, hd_idx=True, hd_d2=True, sigma2=True):
        """-> (nn_idx u32, nn_d2 f32, hd_idx u32, hd_d2 f32, sigma2); an output switched off goes to the library as NULL
        (the result then only stays resident) and comes back as None"""
        n = self.n_rows
        want = (nn_idx, nn_d2, hd_idx, hd_d2)
        out = [np.empty(n, dtype=t) if w else None for w, t in zip(want, (np.uint32, np.float32, np.uint32, np.float32))]
        s2 = C.c_double(0.0)
        capi.check(capi.lib.dc_hip_session_nearest_neighbors(
            self._h, *[a.ctypes.data_as(C.c_void_p) if a is not None else None for a in out],
            C.byref(s2) if sigma2 else None), "dc_hip_session_nearest_neighbors")
        return out[0], out[1], out[2], out[3], (s2.value if sigma2 else None)

    def radius_pairs(self, r2, capacity):
        """dc_hip_session_radius_pairs -> (count of all pairs with d2 < r2, uint32 [min(count, capacity), 2]: the pairs
        written); overwrites the resident populations of device 0"""
        pairs = np.empty((max(capacity, 1), 2), dtype=np.uint32)
        count = C.c_uint64(0)
        capi.check(capi.lib.dc_hip_session_radius_pairs(self._h, float(r2), pairs.ctypes.data_as(C.c_void_p) if capacity else None,
                                                        capacity, C.byref(count)), "dc_hip_session_radius_pairs")
        return int(count.value), pairs[:min(int(count.value), capacity)].copy()

    def radius_forest(self, r2, rank):
        rank = np.ascontiguousarray(rank, dtype=np.uint32)
        assert rank.shape == (self.n_rows,)
        edges = np.empty((max(self.n_rows - 1, 1), 2), dtype=np.uint32)
        n_edges, n_rounds = C.c_size_t(0), C.c_uint32(0)
        capi.check(capi.lib.dc_hip_session_radius_forest(self._h, float(r2), rank.ctypes.data_as(C.c_void_p),
                                                         edges.ctypes.data_as(C.c_void_p), C.byref(n_edges),
                                                         C.byref(n_rounds)), "dc_hip_session_radius_forest")
        return edges[:n_edges.value].copy(), int(n_rounds.value)
