"""CPU: the interface of the pruned wide cross neighbour sweep: the entry point is declared, listed and exported by all
three builds, the ABI number and the variants stay, the workspace query it shares with the pruned cross population sweep
keeps its values, every refusal comes back before a device is touched, naming the function, and the Python functions have
the parameter lists of their unpruned counterparts."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dc_hip_nearest_neighbors_cross_wide_pruned_dev"
INVALID, TOO_LARGE, WORKSPACE = -1, -4, -5


def test_the_symbol_is_declared_and_listed_and_the_abi_number_stays():
    from clustering_amd import capi, density
    text = open(os.path.join(ROOT, "include", "dc_density.h")).read()
    assert re.search(r"DC_API\s+int\s+" + NAME + r"\s*\(", text)
    assert NAME in capi.SYMBOLS and hasattr(capi.lib, NAME)
    assert capi.lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev.argtypes == capi.lib.dc_hip_nearest_neighbors_cross_wide_dev.argtypes
    assert capi.ABI_VERSION == 5 and capi.lib.dc_hip_abi_version() == 5
    assert re.search(r"#define\s+DC_HIP_ABI_VERSION\s+5\b", text)
    assert capi.VARIANTS == {"auto": 0, "direct": 1, "mfma": 2, "pruned": 3, "mfma32": 4, "cross_pruned": 5}
    for fn in ("nearest_reference_wide_pruned", "assign_frames_wide_pruned", "wide_against_pruned_info", "wide_against_pruned_order"):
        assert callable(getattr(density, fn)), fn


@pytest.mark.parametrize("libdir", ["lib", "lib_avx", "lib_fma"])
def test_every_build_exports_the_symbol(libdir):
    path = os.path.join(ROOT, "clustering_amd", libdir, "libdcdensity.so")
    assert os.path.exists(path), "build() makes all three libraries"
    assert hasattr(ctypes.CDLL(path), NAME), libdir


def test_the_workspace_query_keeps_its_values():
    """the neighbour call lives in the arrays the sort leaves free: the six values are those of the library before it"""
    from clustering_amd import capi
    f = capi.lib.dc_hip_cross_wide_pruned_workspace_bytes
    pins = {(1, 1, 65): 116992, (5, 3, 100): 168448, (300, 1500, 100): 1953024, (1500, 300, 256): 4972288,
            (1100, 8320, 80): 8166400, (20000, 200000, 100): 228630784}
    for (n_q, n_r, d), want in pins.items():
        assert f(n_q, n_r, d, 1) == want, (n_q, n_r, d)
    # the words per block -- fe_min per reference block, fe_max, two bounds and the seed per query block -- fit one of the
    # sort's arrays: n_max words, and 64 words (256 bytes) at least
    for n_q, n_r in ((1, 1), (5, 3), (6, 6), (128, 129), (129, 128), (1100, 8320), (20000, 200000), (200000, 20000)):
        words = -(-n_r // 128) + 4 * -(-n_q // 128)
        assert words <= max(max(n_q, n_r), 64), (n_q, n_r)


def test_refusals_come_before_a_device_is_touched():
    from clustering_amd import capi
    lib = capi.lib
    nn = lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev
    fake = ctypes.c_void_p(64)   # never dereferenced: the argument checks come first
    name = NAME.encode()

    def call(n_q=10, n_r=20, d=100, lo=0, hi=10, q=fake, r=fake, fq=fake, fr=fake, out=(fake, fake, fake, fake), ws=fake,
             ws_bytes=1 << 30):
        return nn(q, n_q, r, n_r, d, fq, fr, lo, hi, *out, ws, ws_bytes, None)

    for d in (64, 257, 0, 10):
        assert call(d=d) == INVALID, d
        assert name in lib.dc_hip_last_error()
    # a range that is none of the queries'
    for lo, hi in ((5, 4), (0, 11), (11, 11), (2 ** 40, 2 ** 40 + 1)):
        assert call(lo=lo, hi=hi) == INVALID, (lo, hi)
        assert name in lib.dc_hip_last_error()
    # a workspace one byte short, and none at all
    need = lib.dc_hip_cross_wide_pruned_workspace_bytes(10, 20, 100, 1)
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert name in lib.dc_hip_last_error()
    assert call(ws=None, ws_bytes=0) == WORKSPACE
    assert call(lo=3, hi=3, ws=None) == WORKSPACE, "the workspace check comes before the range is looked at"
    # the unpruned cross sweeps' workspace is too small for the orders
    assert call(n_q=1000, n_r=700, hi=1000, ws_bytes=lib.dc_hip_cross_wide_workspace_bytes(1000, 700, 100, 1)) == WORKSPACE
    # frame ids must fit uint32, and the elements the index arithmetic
    assert call(n_q=2 ** 32, hi=1) == TOO_LARGE
    assert call(n_r=2 ** 32 - 1, hi=1) == TOO_LARGE
    assert call(n_q=2 ** 31, d=256, hi=1) == TOO_LARGE
    assert call(n_r=2 ** 31, d=256, hi=1) == TOO_LARGE
    assert name in lib.dc_hip_last_error()
    # null arrays; with free energies the hd outputs and the reference's free energies are needed as well
    assert call(q=None) == INVALID and call(r=None) == INVALID
    assert call(out=(None, fake, fake, fake)) == INVALID and call(out=(fake, None, fake, fake)) == INVALID
    assert call(out=(fake, fake, None, fake)) == INVALID and call(out=(fake, fake, fake, None)) == INVALID
    assert call(fr=None) == INVALID
    assert name in lib.dc_hip_last_error()


def test_calls_with_nothing_to_write_return_ok():
    from clustering_amd import capi
    nn = capi.lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev
    for d in (65, 256):
        assert nn(None, 0, None, 0, d, None, None, 0, 0, None, None, None, None, None, 0, None) == 0
        assert nn(None, 0, None, 40, d, None, None, 0, 0, None, None, None, None, None, 0, None) == 0   # no queries


def test_the_python_functions_have_the_parameter_lists_of_their_counterparts():
    from clustering_amd import density
    sig = inspect.signature
    assert sig(density.nearest_reference_wide_pruned) == sig(density.nearest_reference_wide)
    params = list(sig(density.assign_frames_wide_pruned).parameters.values())
    assert [p.name for p in params] == ["queries", "reference", "radius", "ref_states", "pruned_neighbours"]
    assert all(p.default is inspect.Parameter.empty for p in params[:4]) and params[4].default is False
    assert list(sig(density.assign_frames_wide).parameters) == ["queries", "reference", "radius", "ref_states"]
