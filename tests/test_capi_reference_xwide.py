"""CPU: the interface of the resident reference for rows of 257..1024 columns (dc_hip_reference_xwide_*),
of dc_hip_assign_open_xwide_dev and of dc_hip_assigner_open_flags: the symbols are declared, listed, bound and exported by
all three builds; the workspace query is zero outside its widths and monotone inside; every refusal that needs no handle
comes back before a device is touched, with fake pointers that are never dereferenced, naming the function.
(The refusals of a handle's state need an open handle, which needs a device: tests/test_gpu_xwide_reference.py.)"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = ("dc_hip_reference_xwide_workspace_bytes", "dc_hip_reference_xwide_open_dev", "dc_hip_reference_xwide_close",
             "dc_hip_reference_xwide_set_free_energies_dev", "dc_hip_reference_xwide_stage_dev",
             "dc_hip_reference_xwide_populations_dev", "dc_hip_reference_xwide_nearest_dev", "dc_hip_reference_xwide_info_dev",
             "dc_hip_reference_xwide_order_dev")
NAMES = REFERENCE + ("dc_hip_assign_open_xwide_dev", "dc_hip_assigner_open_flags")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5
FAKE = 0x10000   # never dereferenced: every call below is refused first


def test_the_symbols_are_declared_listed_and_bound_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in NAMES:
        assert re.search(r"DC_API\s+(int|void|size_t)\s+" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS and getattr(capi.lib, name).argtypes is not None, name
    assert re.search(r"typedef\s+struct\s+dc_reference_xwide\s+dc_reference_xwide\s*;", text)
    assert re.search(r"#define\s+DC_ASSIGNER_XWIDE_REFERENCE\s+0x1u\b", text) and capi.ASSIGNER_XWIDE_REFERENCE == 1
    assert "DC_ASSIGN_XWIDE=1" in text, "the header documents the environment variable"
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    # each entry point has the argument list of its _wide_ namesake
    for name in REFERENCE:
        wide = getattr(capi.lib, name.replace("_xwide_", "_wide_"))
        assert getattr(capi.lib, name).argtypes == wide.argtypes and getattr(capi.lib, name).restype == wide.restype, name
    assert capi.lib.dc_hip_assign_open_xwide_dev.argtypes == capi.lib.dc_hip_assign_open_wide_dev.argtypes
    a, b = capi.lib.dc_hip_assigner_open_flags.argtypes, capi.lib.dc_hip_assigner_open.argtypes
    assert list(a[:-2]) == list(b[:-1]) and a[-2] is ctypes.c_uint and a[-1] == b[-1]
    # the Python class: a Reference with its own three class attributes and one method
    X = density.XWideReference
    assert issubclass(X, density.Reference) and X._api == "dc_hip_reference_xwide_" and X._assign_open == "dc_hip_assign_open_xwide_dev"
    assert X._cols == (257, 1024, "the extra-wide matrix-core sweeps take 257..1024 columns")
    for method in ("stage", "populations", "nearest", "set_free_energies", "info", "order", "assign", "assign_device"):
        assert getattr(X, method) is getattr(density.Reference, method), method
    import inspect
    assert inspect.signature(density.Assigner.__init__).parameters["xwide"].default is False


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_the_workspace_query_is_monotone_and_zero_where_it_should_be():
    from clustering_amd import capi
    f = capi.lib.dc_hip_reference_xwide_workspace_bytes
    sizes = (1, 2, 127, 128, 129, 1000, 1500, 8320, 20000, 100000)
    for d in (0, 1, 64, 65, 256, 1025, 4096):
        assert f(1500, d, 300) == 0, d
    for d in (257, 512, 1024):
        assert f(0, d, 300) == 0 and f(1500, d, 0) == 0
        assert capi.lib.dc_hip_reference_wide_workspace_bytes(1500, d, 300) == 0, "a workspace of one kind never serves the other"
        for fixed in (1, 300, 20000):
            last_r = last_b = 0
            for n in sizes:
                a, b = f(n, d, fixed), f(fixed, d, n)
                assert a >= last_r and b >= last_b and a > 0 and b > 0 and a % 256 == 0, (n, d, fixed)
                last_r, last_b = a, b
    for n_r, n_b in ((1500, 300), (100000, 20000)):
        assert f(n_r, 257, n_b) <= f(n_r, 512, n_b) <= f(n_r, 1024, n_b), "monotone in the columns"
    # the resident form holds what the pruned cross sweep of the same shape holds, and the free energies it keeps
    assert f(100000, 512, 20000) >= capi.lib.dc_hip_cross_xwide_pruned_workspace_bytes(20000, 100000, 512, 1)


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    name = b"dc_hip_reference_xwide_open_dev"

    def open_(d_ref=FAKE, n_ref=1500, n_cols=512, max_batch=300, ws=FAKE, ws_bytes=None, out=True):
        h = ctypes.c_void_p(0x1234)
        need = lib.dc_hip_reference_xwide_workspace_bytes(n_ref, n_cols, max_batch) if ws_bytes is None else ws_bytes
        rc = lib.dc_hip_reference_xwide_open_dev(d_ref, n_ref, n_cols, max_batch, ws, need, None, ctypes.byref(h) if out else None)
        assert rc != 0 and name in lib.dc_hip_last_error(), (rc, lib.dc_hip_last_error())
        assert not out or h.value is None, "*out is NULL on a refusal"
        return rc

    for d in (0, 1, 64, 65, 256, 1025):
        assert open_(n_cols=d, ws_bytes=1 << 30) == INVALID, d
        assert b"257..1024" in lib.dc_hip_last_error(), "the width refusal names the widths of this kind"
    assert open_(n_ref=0, ws_bytes=1 << 30) == INVALID and open_(max_batch=0, ws_bytes=1 << 30) == INVALID
    assert open_(d_ref=None) == INVALID and open_(out=False) == INVALID
    need = lib.dc_hip_reference_xwide_workspace_bytes(1500, 512, 300)
    assert open_(ws_bytes=need - 1) == WORKSPACE and open_(ws=None) == WORKSPACE and open_(ws=None, ws_bytes=0) == WORKSPACE
    assert open_(ws_bytes=lib.dc_hip_cross_xwide_pruned_workspace_bytes(300, 1500, 512, 1)) == WORKSPACE
    assert open_(n_ref=2 ** 32 - 1, ws_bytes=1 << 30) == TOO_LARGE and open_(max_batch=2 ** 32, ws_bytes=1 << 30) == TOO_LARGE
    assert open_(n_ref=2 ** 32 * 4 // 512 + 1, ws_bytes=1 << 30) == TOO_LARGE
    assert open_(max_batch=2 ** 32 * 4 // 512 + 1, ws_bytes=1 << 30) == TOO_LARGE
    # the wide kind still refuses these widths under its own name
    h = ctypes.c_void_p(0x1234)
    assert lib.dc_hip_reference_wide_open_dev(FAKE, 1500, 512, 300, FAKE, 1 << 30, None, ctypes.byref(h)) == INVALID
    assert b"dc_hip_reference_wide_open_dev" in lib.dc_hip_last_error() and b"65..256" in lib.dc_hip_last_error()
    # no handle: every call on one is refused, and close takes a null pointer
    calls = {"dc_hip_reference_xwide_set_free_energies_dev": (FAKE,), "dc_hip_reference_xwide_stage_dev": (FAKE, 10),
             "dc_hip_reference_xwide_populations_dev": (None, 1, FAKE), "dc_hip_reference_xwide_nearest_dev": (None, FAKE, FAKE, None, None),
             "dc_hip_reference_xwide_info_dev": (None, None, None, None, None), "dc_hip_reference_xwide_order_dev": (FAKE, FAKE)}
    for fn, args in calls.items():
        assert getattr(lib, fn)(None, *args, None) == INVALID, fn
        assert fn.encode() in lib.dc_hip_last_error(), fn
    lib.dc_hip_reference_xwide_close(None)


def test_the_assigners_refuse_a_null_reference_and_unknown_flag_bits():
    from clustering_amd import capi
    lib = capi.lib
    out = ctypes.c_void_p(0x1234)
    assert lib.dc_hip_assign_open_xwide_dev(None, FAKE, 10, 1.0, FAKE, 1 << 30, None, ctypes.byref(out)) == INVALID
    assert b"dc_hip_assign_open_xwide_dev" in lib.dc_hip_last_error() and out.value is None
    assert lib.dc_hip_assign_open_xwide_dev(None, FAKE, 10, 1.0, FAKE, 1 << 30, None, None) == INVALID
    for flags in (0x2, 0x3, 0x80000000, 0xFFFFFFFE):
        out = ctypes.c_void_p(0x1234)
        rc = lib.dc_hip_assigner_open_flags(FAKE, 1500, 512, FAKE, 1.0, 300, 0, flags, ctypes.byref(out))
        assert rc == INVALID and b"dc_hip_assigner_open_flags" in lib.dc_hip_last_error() and out.value is None, hex(flags)
    # the known bit passes the flag check: the next refusal is another one, under the same name
    out = ctypes.c_void_p(0x1234)
    assert lib.dc_hip_assigner_open_flags(None, 1500, 512, FAKE, 1.0, 300, 0, 0x1, ctypes.byref(out)) == INVALID
    assert b"null pointer" in lib.dc_hip_last_error() and b"dc_hip_assigner_open_flags" in lib.dc_hip_last_error()
    assert lib.dc_hip_assigner_open_flags(FAKE, 1500, 512, FAKE, 1.0, 300, 0, 0x1, None) == INVALID
