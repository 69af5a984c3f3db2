"""CPU: the interface of the wide sessions and of the neighbour blocks in the order of the pruned wide sweep: the entry
points are declared, listed and exported by all three builds, the ABI number stays, every refusal comes back before a
device is touched with its code and a message, and dc_hip_neighbors_block_rows_wide follows its formula."""
import ctypes
import os
import re

import pytest

import widesessionref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_neighbors_block_rows_wide", "dc_hip_neighbors_block_pack_wide_dev", "dc_hip_neighbors_block_unpack_wide_dev",
         "dc_hip_wide_layout_status_dev", "dc_hip_session_open_flags", "dc_hip_session_wide")
INVALID, NO_DEVICE, TOO_LARGE, WORKSPACE = -1, -2, -4, -5


def test_the_symbols_are_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in NAMES:
        assert re.search(r"DC_API\s+(int|size_t)\s+" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS and hasattr(capi.lib, name), name
    assert re.search(r"#define\s+DC_SESSION_WIDE_SWEEPS\s+0x1u?\b", text) and capi.SESSION_WIDE_SWEEPS == 1
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    for fn in ("neighbor_block_rows_wide", "pack_neighbor_block_wide", "unpack_neighbor_blocks_wide", "wide_layout_status"):
        assert callable(getattr(density, fn)), fn
    assert isinstance(density.Session.wide, property)


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_block_rows_follow_the_formula():
    from clustering_amd import capi, density
    f = capi.lib.dc_hip_neighbors_block_rows_wide
    for n in W.TABLE_ROWS:
        for G in W.TABLE_SEGMENTS:
            for d in (65, 100, 256):
                assert f(n, d, G) == W.block_rows(n, G) == density.neighbor_block_rows_wide(n, d, G), (n, d, G)
    for n in W.BLOCK_ROWS:
        for G in W.BLOCK_SEGMENTS:
            assert f(n, 100, G) == W.block_rows(n, G), (n, G)
    # nothing to pack: no rows, no segments, a width the wide sweeps do not take
    assert f(0, 100, 3) == 0 and f(300, 100, 0) == 0 and f(300, 64, 3) == 0 and f(300, 257, 3) == 0


def test_pack_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    pack = lib.dc_hip_neighbors_block_pack_wide_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    name = b"dc_hip_neighbors_block_pack_wide_dev"
    big = 1 << 30
    args = lambda **kw: [kw.get("a", fake), fake, fake, fake, kw.get("n", 10), kw.get("d", 100), kw.get("seg", 0), kw.get("G", 2),
                         kw.get("ws", fake), kw.get("bytes", big), kw.get("block", fake), None]
    for seg, G in ((2, 2), (7, 3), (0, 0), (5, 0), (2 ** 40, 5)):
        assert pack(*args(seg=seg, G=G)) == INVALID, (seg, G)
        assert name in lib.dc_hip_last_error()
    for d in (64, 257, 0, 10):
        assert pack(*args(d=d)) == INVALID, d
        assert name in lib.dc_hip_last_error()
    need = lib.dc_hip_wide_pruned_workspace_bytes(10, 100, 1)
    assert pack(*args(bytes=need - 1)) == WORKSPACE and name in lib.dc_hip_last_error()
    assert pack(*args(ws=None, bytes=0)) == WORKSPACE and pack(*args(ws=None)) == WORKSPACE
    assert pack(*args(n=1000, bytes=lib.dc_hip_wide_workspace_bytes(1000, 100, 1))) == WORKSPACE, "the unpruned sweeps' workspace holds no order"
    assert pack(*args(n=2 ** 32)) == TOO_LARGE and name in lib.dc_hip_last_error()
    assert pack(*args(a=None)) == INVALID and pack(*args(block=None)) == INVALID
    # no rows: nothing to pack, whatever else is passed
    for d in (65, 256):
        assert pack(None, None, None, None, 0, d, 1, 3, None, 0, None, None) == 0


def test_unpack_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    unpack = lib.dc_hip_neighbors_block_unpack_wide_dev
    fake = ctypes.c_void_p(64)
    name = b"dc_hip_neighbors_block_unpack_wide_dev"
    big = 1 << 30
    args = lambda **kw: [kw.get("blocks", fake), kw.get("n", 10), kw.get("d", 100), kw.get("G", 2), kw.get("ws", fake),
                         kw.get("bytes", big), kw.get("a", fake), fake, fake, fake, None]
    assert unpack(*args(G=0)) == INVALID and name in lib.dc_hip_last_error()
    for d in (64, 257, 0, 10):
        assert unpack(*args(d=d)) == INVALID, d
        assert name in lib.dc_hip_last_error()
    need = lib.dc_hip_wide_pruned_workspace_bytes(10, 100, 1)
    assert unpack(*args(bytes=need - 1)) == WORKSPACE and name in lib.dc_hip_last_error()
    assert unpack(*args(ws=None, bytes=0)) == WORKSPACE
    assert unpack(*args(n=2 ** 32)) == TOO_LARGE
    assert unpack(*args(blocks=None)) == INVALID and unpack(*args(a=None)) == INVALID
    assert unpack(None, 0, 100, 3, None, 0, None, None, None, None, None) == 0
    # the status query: null arguments
    assert lib.dc_hip_wide_layout_status_dev(None, None, None) == INVALID
    assert b"dc_hip_wide_layout_status_dev" in lib.dc_hip_last_error()
    assert lib.dc_hip_wide_layout_status_dev(fake, None, None) == INVALID


def test_session_flags_are_checked_before_a_device_is_touched():
    import numpy as np
    from clustering_amd import capi
    lib = capi.lib
    c = np.zeros((8, 100), dtype=np.float32)
    h = ctypes.c_void_p(0)
    p = c.ctypes.data_as(ctypes.c_void_p)
    for flags in (0x2, 0x3, 0x80000000):
        assert lib.dc_hip_session_open_flags(p, 8, 100, None, 0, flags, ctypes.byref(h)) == INVALID and not h.value, flags
        assert b"flags" in lib.dc_hip_last_error()
    assert lib.dc_hip_session_open_flags(p, 8, 100, None, 0, 1, None) == INVALID
    assert lib.dc_hip_session_open_flags(p, 8, 0, None, 0, 1, ctypes.byref(h)) == INVALID      # n_cols = 0, as dc_hip_session_open
    assert lib.dc_hip_session_wide(None) == 0
    if capi.device_count() == 0:      # known flags on a box without a GPU: a status and a message, never a crash or a CPU path
        for flags in (0, 1):
            assert lib.dc_hip_session_open_flags(p, 8, 100, None, 0, flags, ctypes.byref(h)) == NO_DEVICE and not h.value
            assert b"no HIP device" in lib.dc_hip_last_error()
