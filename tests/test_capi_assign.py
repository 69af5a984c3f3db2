"""CPU: the assigner's entry points (dc_hip_assign_*, dc_hip_assigner_*) and `clustering assign` as far as they go without a
device -- symbols, prototypes, the workspace size, refusals, option parsing and help."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "clustering_amd", "bin", "clustering")
NEW = ("dc_hip_assign_workspace_bytes", "dc_hip_assign_open_dev", "dc_hip_assign_open_wide_dev", "dc_hip_assign_close",
       "dc_hip_assign_batch_dev", "dc_hip_assigner_open", "dc_hip_assigner_reference", "dc_hip_assigner_path",
       "dc_hip_assigner_assign", "dc_hip_assigner_close")
INVALID, NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def capi():
    from clustering_amd import capi
    return capi


def test_symbols_and_prototypes(capi):
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    for name in NEW:
        assert name in capi.SYMBOLS and "DC_API" in text and name + "(" in text, name
        fn = getattr(capi.lib, name)
        assert fn.argtypes is not None, name
    assert capi.lib.dc_hip_assign_workspace_bytes.restype is C.c_size_t
    assert capi.lib.dc_hip_assign_close.restype is None and capi.lib.dc_hip_assigner_close.restype is None
    assert len(capi.lib.dc_hip_assign_batch_dev.argtypes) == 11 and len(capi.lib.dc_hip_assigner_assign.argtypes) == 10
    assert len(capi.lib.dc_hip_assign_open_dev.argtypes) == len(capi.lib.dc_hip_assign_open_wide_dev.argtypes) == 8
    assert len(capi.lib.dc_hip_assigner_open.argtypes) == 8
    assert capi.lib.dc_hip_abi_version() == 5, "additive: the ABI number stays"


def test_workspace_bytes(capi):
    size = capi.lib.dc_hip_assign_workspace_bytes
    assert size(0, 100) == 0 and size(100, 0) == 0 and size(0, 0) == 0
    counts = (1, 2, 33, 1500, 1501, 10**6)
    for a in counts:
        for b in counts:
            # the table [n_ref + 1], the states [n_ref], six arrays [max_batch]
            assert size(a, b) >= 4 * (a + 1) + 4 * a + 6 * 4 * b
    for n in counts:
        row = [size(n, b) for b in counts]
        col = [size(a, n) for a in counts]
        assert row == sorted(row) and col == sorted(col), "monotone in both arguments"


def test_null_handles_are_refused(capi):
    lib, h = capi.lib, C.c_void_p(0x1)
    for fn in (lib.dc_hip_assign_open_dev, lib.dc_hip_assign_open_wide_dev):
        h.value = 0x1
        assert fn(None, None, 1, 1.0, None, 0, None, C.byref(h)) == INVALID and not h.value, "*out is NULL on a refusal"
        assert fn.__name__ in lib.dc_hip_last_error().decode()
        assert fn(None, None, 1, 1.0, None, 0, None, None) == INVALID
    assert lib.dc_hip_assign_batch_dev(None, None, 0, None, None, None, None, None, None, None, None) == INVALID
    assert "dc_hip_assign_batch_dev" in lib.dc_hip_last_error().decode()
    assert lib.dc_hip_assigner_assign(None, None, 0, None, None, None, None, None, None, None) == INVALID
    assert lib.dc_hip_assigner_reference(None, None, None, None) == INVALID
    assert lib.dc_hip_assigner_path(None) == -1
    lib.dc_hip_assign_close(None)      # closing nothing is a no-op
    lib.dc_hip_assigner_close(None)


def test_assigner_open_refusals_and_no_device(capi):
    lib = capi.lib
    ref = np.zeros((8, 3), np.float32)
    states = np.zeros(8, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p(0x1)
    for args in ((None, 8, 3, p(states), 1.0, 4), (p(ref), 8, 3, None, 1.0, 4), (p(ref), 0, 3, p(states), 1.0, 4),
                 (p(ref), 8, 0, p(states), 1.0, 4), (p(ref), 8, 3, p(states), 1.0, 0), (p(ref), 8, 3, p(states), -1.0, 4),
                 (p(ref), 8, 3, p(states), float("nan"), 4)):
        h.value = 0x1
        assert lib.dc_hip_assigner_open(*args, 0, C.byref(h)) == INVALID and not h.value, args
        assert "dc_hip_assigner_open" in lib.dc_hip_last_error().decode()
    assert lib.dc_hip_assigner_open(p(ref), 8, 3, p(states), 1.0, 4, 0, None) == INVALID
    if capi.device_count() > 0:
        return   # (with a device the call opens: tests/test_gpu_assign.py)
    h.value = 0x1
    assert lib.dc_hip_assigner_open(p(ref), 8, 3, p(states), 1.0, 4, 0, C.byref(h)) == NO_DEVICE and not h.value
    assert b"no HIP device" in lib.dc_hip_last_error()


def run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def test_cli_lists_both_modes():
    r = run()
    assert r.returncode != 0
    assert "density:" in r.stderr and "assign:" in r.stderr and "clustering density -h" in r.stderr and "clustering assign -h" in r.stderr


def test_cli_assign_help_lists_its_options():
    r = run("assign", "-h")
    assert r.returncode == 0
    for opt in ("--file", "--states", "--query", "--radius", "--output", "--population", "--free-energy", "--nearest-neighbors",
                "--batch", "--verbose"):
        assert opt in r.stdout, opt
    d = run("density", "-h")
    assert d.returncode == 0 and "--states" not in d.stdout and "--radii" in d.stdout, "the density help is its own"


@pytest.mark.parametrize("missing, name", [("-f", "--file"), ("-q", "--query"), ("-s", "--states"), ("-o", "--output"), ("-r", "--radius")])
def test_cli_assign_names_the_missing_option(missing, name):
    args = {"-f": "ref", "-q": "new", "-s": "states", "-o": "out", "-r": "0.5"}
    del args[missing]
    r = run("assign", *[x for kv in args.items() for x in kv])
    assert r.returncode != 0 and f"'{name}' is required" in r.stderr, r.stderr[:300]


def test_cli_assign_refuses_unknown_options_and_a_bad_batch():
    r = run("assign", "-f", "x", "--frobnicate")
    assert r.returncode != 0 and "unrecognised option '--frobnicate'" in r.stderr
    r = run("assign", "-f", "x", "--batch", "0")
    assert r.returncode != 0 and "--batch" in r.stderr
    r = run("assign", "-f", "x", "-q")
    assert r.returncode != 0 and "'--query' is missing" in r.stderr


def test_cli_assign_without_a_gpu_says_so(tmp_path, capi):
    if capi.device_count() > 0:
        return
    r = run("assign", "-f", "ref", "-q", "new", "-s", "states", "-o", str(tmp_path / "out"), "-r", "0.5")
    assert r.returncode != 0 and "no HIP-compatible GPUs found" in r.stderr
    assert not (tmp_path / "out").exists()
