"""GPU: the fp32-input matrix-core sweeps for rows of 1..32 columns with several radii per sweep
(density.calculate_populations_fp32 / nearest_neighbors_fp32) against the CPU oracle, bit for bit: populations, free
energies, nn_idx, nn_d2 bits, hd_idx, hd_d2 bits.  Cases: tests/fp32ref.py (their premises are asserted on the CPU by
tests/test_fp32_cases.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import fe_families
import fp32ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available()
    from clustering_amd import density
    return density


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(t):
    return t.cpu().numpy().astype(np.uint32).astype(np.uint64)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def reference(n_rows, n_cols, k=1):
    """(coords, radii, populations, free energies of the first radius, neighbours): computed once per shape"""
    from oracle.oracle import Oracle
    o = Oracle()
    c = fp32ref.blobs(n_rows, n_cols)
    radii = fp32ref.radii_for(c, k)
    pops = o.populations(c, radii)
    fe = o.free_energies(pops[0])
    return c, radii, pops, fe, o.nearest_neighbors(c, fe)


def answered_by(dens, device):
    """which kernel answered the last fp32 call on this device: header word 1 of its workspace is the device-side gate --
    0: the matrix-core sweep ran and the direct kernel left at once, anything else: the other way round"""
    word = int(dens._cached("fp32", device).buf[4:8].view(__import__("torch").int32).item())
    return "direct" if word else "mfma"


def check_pops(dens, oracle, c, radii, lo=None, hi=None, want=None, path="mfma"):
    ct = dev(c)
    got = dens.calculate_populations_fp32(ct, radii, lo, hi)
    if (len(c) if hi is None else hi) > (0 if lo is None else lo):
        assert answered_by(dens, ct.device) == path, "a silent fall-back to the direct kernel would pass every comparison"
    if want is None:
        want = oracle.populations(c, radii, 0 if lo is None else lo, hi)
    assert got.shape == (len(radii), len(c))
    assert (u64(got) == want).all(), ("populations", c.shape, radii, lo, hi)
    return got


def check_nn(dens, oracle, c, fe, lo=None, hi=None, want=None, path="mfma"):
    ct = dev(c)
    got = dens.nearest_neighbors_fp32(ct, dev(np.asarray(fe, dtype=np.float32)), lo, hi)
    if (len(c) if hi is None else hi) > (0 if lo is None else lo):
        assert answered_by(dens, ct.device) == ("direct" if np.isnan(fe).any() else path)   # (a NaN free energy flags the sweep)
    if want is None:
        want = oracle.nearest_neighbors(c, fe, 0 if lo is None else lo, hi)
    assert (u64(got[0]) == want[0]).all(), ("nn_idx", c.shape, lo, hi)
    assert (bits(got[1].cpu().numpy()) == bits(want[1])).all(), ("nn_d2", c.shape, lo, hi)
    assert (u64(got[2]) == want[2]).all(), ("hd_idx", c.shape, lo, hi)
    assert (bits(got[3].cpu().numpy()) == bits(want[3])).all(), ("hd_d2", c.shape, lo, hi)


@pytest.mark.parametrize("n_rows", fp32ref.ROWS)
@pytest.mark.parametrize("n_cols", fp32ref.COLS)
def test_populations_free_energies_and_neighbours_at_every_width_and_row_count(dens, oracle, n_cols, n_rows):
    c, radii, pops, fe, nn = reference(n_rows, n_cols)
    got = check_pops(dens, oracle, c, radii, want=pops)
    fe_got = dens.calculate_free_energies(got[0].contiguous())
    assert (bits(fe_got.cpu().numpy()) == bits(fe)).all(), ("free energies", n_rows, n_cols)
    check_nn(dens, oracle, c, fe, want=nn)
    if n_rows == 1:
        assert int(pops[0][0]) == 1 and int(nn[0][0]) == 2 and nn[1][0] == FLT_MAX


@pytest.mark.parametrize("n_cols", (5, 10, 16, 30))
@pytest.mark.parametrize("name", sorted(fp32ref.radius_sets(fp32ref.blobs(600, 5))))
def test_radius_sets_in_the_callers_order(dens, oracle, name, n_cols):
    c = fp32ref.blobs(600, n_cols)
    radii = fp32ref.radius_sets(c)[name]
    want = oracle.populations(c, radii)
    got = check_pops(dens, oracle, c, radii, want=want)
    for k, r in enumerate(radii):   # each row equals the one-radius call of that radius
        one = dens.calculate_populations_fp32(dev(c), [r])
        assert (one[0] == got[k]).all(), (name, n_cols, k, r)
    if name == "nine":
        assert any((want[k] != want[k + 1]).any() for k in range(len(radii) - 1)), "populations differ between adjacent radii"


@pytest.mark.parametrize("lo,hi", [(137, 411), (300, 300), (311, 312), (0, 1), (599, 600), (32, 64)])
@pytest.mark.parametrize("n_cols", (5, 30))
def test_row_ranges(dens, oracle, n_cols, lo, hi):
    c, _, _, fe, _ = reference(600, n_cols)
    check_pops(dens, oracle, c, fp32ref.radii_for(c, 3), lo, hi)
    check_nn(dens, oracle, c, fe, lo, hi)


@pytest.mark.parametrize("n_cols", (1, 2, 5, 10, 30))
def test_lattice_pairs_exactly_on_the_radius_are_outside(dens, oracle, n_cols):
    c, radii = fp32ref.lattice_case(n_cols)
    check_pops(dens, oracle, c, radii)
    for r in radii:
        check_pops(dens, oracle, c, [r])


@pytest.mark.parametrize("n_cols", (3, 5, 10, 17, 30))
def test_band_pairs_of_the_smallest_and_the_largest_radius(dens, oracle, n_cols):
    c, radii, _ = fp32ref.band_case(600, n_cols)
    check_pops(dens, oracle, c, radii)
    check_pops(dens, oracle, c, radii[::-1])


@pytest.mark.parametrize("n_cols", (2, 5, 9, 30))
def test_ties_the_lowest_index_wins(dens, oracle, n_cols):
    c = fp32ref.tie_case(n_cols)
    radii = fp32ref.radii_for(c, 2)
    pops = oracle.populations(c, radii)
    check_pops(dens, oracle, c, radii, want=pops)
    for family in ("pops", "constant", "ties_ulp"):
        check_nn(dens, oracle, c, fe_families.make(family, c, pops[0]))


@pytest.mark.parametrize("n_cols", (5, 10, 30))
def test_a_chain_that_passes_the_tile_test_of_the_largest_radius_only(dens, oracle, n_cols):
    c, radii = fp32ref.tile_test_case(n_cols)
    want = oracle.populations(c, radii)
    assert (want[0] == 1).all() and (want[1] == len(c)).all()
    check_pops(dens, oracle, c, radii, want=want)
    check_pops(dens, oracle, c, radii[::-1], want=want[::-1])


@pytest.mark.parametrize("factor", (1e-12, 1e15))
@pytest.mark.parametrize("n_cols", (5, 30))
def test_scaled_data_with_radii_scaled_along(dens, oracle, n_cols, factor):
    base = fp32ref.blobs(600, n_cols)
    c = np.ascontiguousarray((base.astype(np.float64) * factor).astype(np.float32))
    radii = [float(np.float32(r * factor)) for r in fp32ref.radii_for(base, 3)]
    pops = oracle.populations(c, radii)
    check_pops(dens, oracle, c, radii, want=pops)
    check_nn(dens, oracle, c, oracle.free_energies(pops[0]))


@pytest.mark.parametrize("n_cols", (1, 5, 30))
def test_all_rows_equal(dens, oracle, n_cols):
    c = np.full((257, n_cols), 0.375, dtype=np.float32)
    radii = [0.0, 1.0, float("inf")]
    pops = oracle.populations(c, radii)
    check_pops(dens, oracle, c, radii, want=pops)
    check_nn(dens, oracle, c, oracle.free_energies(pops[1]))


@pytest.mark.parametrize("what", ("nan", "inf", "overflow"))
@pytest.mark.parametrize("n_cols", (5, 30))
def test_flagged_data_takes_the_gated_direct_path(dens, oracle, n_cols, what):
    c = np.array(fp32ref.blobs(257, n_cols))
    if what == "overflow":
        c[100] = 3.0e19     # |x'|^2 overflows the Gram form, the canonical distance is finite or inf as the oracle has it
    else:
        c[100, n_cols // 2] = {"nan": np.nan, "inf": np.inf}[what]
    radii = fp32ref.radii_for(fp32ref.blobs(257, n_cols), 3)
    pops = oracle.populations(c, radii)
    check_pops(dens, oracle, c, radii, want=pops, path="direct")
    check_nn(dens, oracle, c, oracle.free_energies(pops[0]), path="direct")


@pytest.mark.parametrize("family", sorted(fe_families.FAMILIES))
@pytest.mark.parametrize("n_cols", (5, 10, 30))
def test_neighbours_with_free_energies_of_any_origin(dens, oracle, n_cols, family):
    c, _, pops, _, _ = reference(600, n_cols)
    fe = fe_families.make(family, c, pops[0])
    check_nn(dens, oracle, c, fe)
    check_nn(dens, oracle, c, fe, 137, 411)


CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import fp32ref
from clustering_amd import density
from oracle.oracle import Oracle
o = Oracle()
for d in (5, 30):
    c = fp32ref.blobs(1500, d)
    radii = fp32ref.radii_for(c, 3)
    assert density.fp32_sweep_plan(1500, d, 3)["chunks_pop"] == 3 and density.fp32_sweep_plan(1500, d, 3)["chunks_nn"] == 3
    ct = torch.from_numpy(c).cuda()
    want = o.populations(c, radii)
    got = density.calculate_populations_fp32(ct, radii)
    assert (got.cpu().numpy().astype(np.uint32).astype(np.uint64) == want).all(), ("pops", d)
    fe = o.free_energies(want[0])
    nn = density.nearest_neighbors_fp32(ct, torch.from_numpy(fe).cuda())
    exp = o.nearest_neighbors(c, fe)
    for k in (0, 2):
        assert (nn[k].cpu().numpy().astype(np.uint32).astype(np.uint64) == exp[k]).all(), ("idx", d, k)
    for k in (1, 3):
        assert (nn[k].cpu().numpy().view(np.uint32) == exp[k].view(np.uint32)).all(), ("d2", d, k)
print("CHUNKS OK")
"""


POISON = """
import sys
import numpy as np
import torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import fp32ref
from clustering_amd import density
from oracle.oracle import Oracle
o = Oracle()
for d in (1, 3, 5, 7, 9, 11, 13, 17, 21, 25, 29, 30, 31):
    c = fp32ref.blobs(300, d)
    ct = torch.from_numpy(np.array(c)).cuda()
    for k in (1, 3):
        radii = fp32ref.radii_for(c, k)
        want = o.populations(c, radii)
        got = density.calculate_populations_fp32(ct, radii)
        assert (got.cpu().numpy().astype(np.uint32).astype(np.uint64) == want).all(), ("pops", d, k)
    assert int(density._cached("fp32", ct.device).buf[4:8].view(torch.int32).item()) == 0, "the matrix-core sweep answered"
    fe = o.free_energies(want[0])
    nn = density.nearest_neighbors_fp32(ct, torch.from_numpy(fe).cuda())
    exp = o.nearest_neighbors(c, fe)
    for k in (0, 2):
        assert (nn[k].cpu().numpy().astype(np.uint32).astype(np.uint64) == exp[k]).all(), ("idx", d, k)
    for k in (1, 3):
        assert (nn[k].cpu().numpy().view(np.uint32) == exp[k].view(np.uint32)).all(), ("d2", d, k)
print("POISON OK")
"""


def test_no_kernel_reads_a_pad_float_of_the_image():
    """The pad floats of a lane and the unused half of an odd width's last step are zeros, so a fragment read from the wrong
    one of them changes no result.  DC_MFMA32_POISON_PADS=1 (a fresh process: the switches are read once) makes the image
    pass write NaN into every pad float: results stay those of the oracle only if no chain ever multiplies one -- at odd
    widths of every instance that has pads, one and several radii, both sweeps."""
    env = dict(os.environ, DC_MFMA32_POISON_PADS="1")
    r = subprocess.run([sys.executable, "-c", POISON.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "POISON OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_reference_chunks_in_a_fresh_process(oracle):
    env = dict(os.environ, DC_MFMA32_CHUNKS="3")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CHUNKS OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("n_cols", (9, 10))
@pytest.mark.parametrize("n_rows", (33, 600, 3000))
def test_at_9_and_10_columns_one_radius_equals_variant_mfma32(dens, oracle, n_cols, n_rows):
    c, radii, pops, fe, nn = reference(n_rows, n_cols)
    ct, ft = dev(c), dev(fe)
    a = dens.calculate_populations_fp32(ct, radii)
    b = dens.calculate_populations_partial(ct, radii, variant="mfma32")
    assert (a == b).all() and (u64(a) == pops).all()
    x = dens.nearest_neighbors_fp32(ct, ft)
    y = dens.nearest_neighbors_partial(ct, ft, variant="mfma32")
    for k in range(4):
        assert (x[k].cpu().numpy().view(np.uint32) == y[k].cpu().numpy().view(np.uint32)).all(), k


def test_fuzz_against_the_direct_variant(dens):
    import torch
    for n_rows, n_cols, n_radii, seed in fp32ref.fuzz_shapes():
        c = fp32ref.blobs(n_rows, n_cols, seed=seed)
        radii = fp32ref.radii_for(c, n_radii)
        ct = dev(c)
        a = dens.calculate_populations_fp32(ct, radii)
        b = dens.calculate_populations_partial(ct, radii, variant="direct")
        assert (a == b).all(), ("populations", n_rows, n_cols, n_radii, seed)
        fe = dens.calculate_free_energies(b[0].contiguous())
        x = dens.nearest_neighbors_fp32(ct, fe)
        y = dens.nearest_neighbors_partial(ct, fe, variant="direct")
        for k in range(4):
            assert torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), ("neighbours", k, n_rows, n_cols, seed)
