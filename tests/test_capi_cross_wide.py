"""CPU: the interface of the cross form of the wide matrix-core sweeps (queries against a reference at 65..256 columns):
the three entry points are declared, listed and exported by all three builds, the ABI number and the variant table stay,
the workspace query follows its rule, the refusals come back before a device is touched and name the function, and the
Python functions exist and refuse other column counts."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dc_hip_cross_wide_workspace_bytes", "dc_hip_populations_cross_wide_dev", "dc_hip_nearest_neighbors_cross_wide_dev")
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5


def nm_for(d):
    return (3 * d + 2 + 15) // 16


def test_the_symbols_are_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    assert re.search(r"DC_API\s+size_t\s+" + NAMES[0] + r"\s*\(", text)
    for name in NAMES[1:]:
        assert re.search(r"DC_API\s+int\s+" + name + r"\s*\(", text), name
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib, name), name
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    # no variant value of its own
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}
    # the info call says that it serves the cross-wide workspace too
    info = text[text.index("the last wide sweep CALL"):text.index("DC_API int dc_hip_wide_info_dev")]
    assert "cross_wide" in info


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbols(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    lib = ctypes.CDLL(path)
    for name in NAMES:
        assert hasattr(lib, name), (libdir, name)


def test_workspace_rule():
    from clustering_amd import capi
    f = capi.lib.dc_hip_cross_wide_workspace_bytes
    for d in (1, 10, 64, 257, 400, 1000):
        for n_q, n_r in ((1, 1), (1000, 1000), (20000, 200000)):
            assert f(n_q, n_r, d, 1) == 0, (n_q, n_r, d)
    sizes = [1, 31, 32, 33, 127, 128, 129, 1000, 1001, 4096, 100000, 1000000]
    for d in (65, 100, 128, 256):
        assert f(0, 1000, d, 1) == 0 and f(1000, 0, d, 1) == 0 and f(0, 0, d, 1) == 0, "an empty side needs no workspace"
        for other in (1, 1000):
            by_q = [f(n, other, d, 1) for n in sizes]
            by_r = [f(other, n, d, 1) for n in sizes]
            assert by_q[0] > 0 and by_q == sorted(by_q) and by_q[-1] > by_q[0], ("monotone in n_query", d)
            assert by_r[0] > 0 and by_r == sorted(by_r) and by_r[-1] > by_r[0], ("monotone in n_ref", d)
        assert f(1000, 3000, d, 9) == f(1000, 3000, d, 1)
        # both operand images (16 bytes x 64 lanes per MFMA and 32-row tile of either set) and the merge words
        for n_q, n_r in ((1, 1), (130, 1100), (2100, 40), (20000, 200000)):
            images = 1024 * nm_for(d) * (-(-n_q // 32) + -(-n_r // 32))
            assert f(n_q, n_r, d, 1) >= images + 16 * n_q, (n_q, n_r, d)
    assert f(1000, 1000, 256, 1) > f(1000, 1000, 65, 1)
    # a reference image is not paid for by the queries' rows, nor the other way round
    assert f(100, 100000, 100, 1) < f(100000, 100000, 100, 1) and f(100000, 100, 100, 1) < f(100000, 100000, 100, 1)
    # the pins of the existing queries stay
    assert capi.lib.dc_hip_cross_workspace_bytes(1000, 1000, 100) == 0
    assert capi.lib.dc_hip_wide_workspace_bytes(1000, 64, 1) == 0 and capi.lib.dc_hip_wide_workspace_bytes(1000, 100, 1) > 0


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    pop, nn = lib.dc_hip_populations_cross_wide_dev, lib.dc_hip_nearest_neighbors_cross_wide_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    rad = (ctypes.c_float * 1)(0.5)
    big = 1 << 30
    for d in (64, 257, 0, 10):
        assert pop(fake, 10, fake, 10, d, rad, 1, 0, 10, fake, fake, big, None) == INVALID, d
        assert b"dc_hip_populations_cross_wide_dev" in lib.dc_hip_last_error()
        assert nn(fake, 10, fake, 10, d, fake, fake, 0, 10, fake, fake, fake, fake, fake, big, None) == INVALID, d
        assert b"dc_hip_nearest_neighbors_cross_wide_dev" in lib.dc_hip_last_error()
    # a workspace one byte short, and none at all
    need = lib.dc_hip_cross_wide_workspace_bytes(10, 20, 100, 1)
    assert pop(fake, 10, fake, 20, 100, rad, 1, 0, 10, fake, fake, need - 1, None) == WORKSPACE
    assert b"dc_hip_populations_cross_wide_dev" in lib.dc_hip_last_error()
    assert pop(fake, 10, fake, 20, 100, rad, 1, 0, 10, fake, None, 0, None) == WORKSPACE
    assert nn(fake, 10, fake, 20, 100, fake, fake, 0, 10, fake, fake, fake, fake, fake, need - 1, None) == WORKSPACE
    assert b"dc_hip_nearest_neighbors_cross_wide_dev" in lib.dc_hip_last_error()
    assert nn(fake, 10, fake, 20, 100, None, None, 0, 10, fake, fake, None, None, None, 0, None) == WORKSPACE
    # frame ids must fit uint32 on either side; row ranges inside the QUERY rows
    assert pop(fake, 2 ** 32, fake, 10, 100, rad, 1, 0, 10, fake, fake, big, None) == TOO_LARGE
    assert pop(fake, 10, fake, 2 ** 32 - 1, 100, rad, 1, 0, 10, fake, fake, big, None) == TOO_LARGE
    assert nn(fake, 2 ** 32, fake, 10, 100, fake, fake, 0, 10, fake, fake, fake, fake, fake, big, None) == TOO_LARGE
    assert nn(fake, 10, fake, 2 ** 32 - 1, 100, fake, fake, 0, 10, fake, fake, fake, fake, fake, big, None) == TOO_LARGE
    assert pop(fake, 10, fake, 20, 100, rad, 1, 5, 4, fake, fake, big, None) == INVALID
    assert pop(fake, 10, fake, 20, 100, rad, 1, 0, 11, fake, fake, big, None) == INVALID
    assert nn(fake, 10, fake, 20, 100, fake, fake, 0, 11, fake, fake, fake, fake, fake, big, None) == INVALID
    assert nn(fake, 10, fake, 20, 100, fake, fake, 0, 20, fake, fake, fake, fake, fake, big, None) == INVALID, "i_to counts query rows"
    # null arrays
    assert pop(None, 10, fake, 20, 100, rad, 1, 0, 10, fake, fake, big, None) == INVALID
    assert pop(fake, 10, None, 20, 100, rad, 1, 0, 10, fake, fake, big, None) == INVALID
    assert pop(fake, 10, fake, 20, 100, None, 1, 0, 10, fake, fake, big, None) == INVALID
    assert pop(fake, 10, fake, 20, 100, rad, 1, 0, 10, None, fake, big, None) == INVALID
    assert nn(None, 10, fake, 20, 100, fake, fake, 0, 10, fake, fake, fake, fake, fake, big, None) == INVALID
    assert nn(fake, 10, None, 20, 100, fake, fake, 0, 10, fake, fake, fake, fake, fake, big, None) == INVALID
    assert nn(fake, 10, fake, 20, 100, fake, fake, 0, 10, None, fake, fake, fake, fake, big, None) == INVALID
    # free energies of the queries ask for those of the reference and for the hd outputs
    assert nn(fake, 10, fake, 20, 100, fake, None, 0, 10, fake, fake, fake, fake, fake, big, None) == INVALID
    assert nn(fake, 10, fake, 20, 100, fake, fake, 0, 10, fake, fake, None, fake, fake, big, None) == INVALID
    assert nn(fake, 10, fake, 20, 100, fake, fake, 0, 10, fake, fake, fake, None, fake, big, None) == INVALID


def test_calls_with_nothing_to_write_return_ok():
    from clustering_amd import capi
    lib = capi.lib
    rad = (ctypes.c_float * 1)(0.5)
    fake = ctypes.c_void_p(64)
    for d in (65, 256):
        assert lib.dc_hip_populations_cross_wide_dev(None, 0, fake, 10, d, rad, 1, 0, 0, None, None, 0, None) == 0
        assert lib.dc_hip_populations_cross_wide_dev(None, 0, None, 0, d, rad, 1, 0, 0, None, None, 0, None) == 0
        assert lib.dc_hip_populations_cross_wide_dev(None, 10, None, 10, d, rad, 0, 0, 10, None, None, 0, None) == 0   # no radii
        assert lib.dc_hip_nearest_neighbors_cross_wide_dev(None, 0, fake, 10, d, None, None, 0, 0, None, None, None, None, None,
                                                           0, None) == 0


def test_the_python_functions_exist_and_refuse_other_column_counts():
    import inspect

    import torch
    from clustering_amd import density
    assert list(inspect.signature(density.calculate_populations_against_wide).parameters) == \
        ["queries", "reference", "radii", "i_from", "i_to", "out"]
    assert list(inspect.signature(density.nearest_reference_wide).parameters) == \
        ["queries", "reference", "fe_query", "fe_ref", "i_from", "i_to"]
    assert list(inspect.signature(density.assign_frames_wide).parameters) == ["queries", "reference", "radius", "ref_states"]
    assert density.wide_against_info("cuda:0") == (0, 0, 0), "before any call: no workspace, no device touched"
    for d in (10, 64, 257, 400):
        q, r = torch.zeros((4, d)), torch.zeros((6, d))
        with pytest.raises(ValueError, match="65..256"):
            density.calculate_populations_against_wide(q, r, [0.5])
        with pytest.raises(ValueError, match="65..256"):
            density.nearest_reference_wide(q, r)
        with pytest.raises(ValueError, match="65..256"):
            density.assign_frames_wide(q, r, 0.5, [0] * 6)
    # assign_frames keeps its signature
    assert list(inspect.signature(density.assign_frames).parameters) == \
        ["queries", "reference", "radius", "ref_states", "variant", "pruned_neighbours"]
