"""CPU: the premises of the cases of tests/test_gpu_xwide.py (tests/xwideref.py): the column counts cover every NM mod 4, the
first chain longer than the 65..256 sweeps ran, both fallback kernels and the maximum; the row counts reach two reference
shares; the Python restatement of scale and band is the product's own; and the cap the GPU test holds the exact-path
counter to is a small share of the pairs, so that a sweep which defers everything cannot meet it."""
import os
import subprocess

import numpy as np
import pytest

import xwideref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_column_counts_cover_every_chunk_remainder_the_fallback_seam_and_the_maximum():
    nm = {d: xwideref.nm_for(d) for d in xwideref.COLS}
    assert (nm[257], nm[261], nm[267], nm[272]) == (49, 50, 51, 52)
    assert {nm[d] % xwideref.KC for d in (257, 261, 267, 272)} == {0, 1, 2, 3}
    assert xwideref.nm_for(256) == 49 and nm[258] == 49 and nm[261] == 49 + 1, "261: the first chain beyond the old maximum"
    assert 400 in xwideref.COLS and 401 in xwideref.COLS, "the generic direct kernel ends at 400 columns, the chunked one starts at 401"
    assert min(xwideref.COLS) == xwideref.MIN_COLS and max(xwideref.COLS) == xwideref.MAX_COLS
    assert nm[1024] == 193 and xwideref.nb_ns(1024) == (65, 128)
    assert nm[1023] == 192, "both sides of the last MFMA"
    assert all(xwideref.MIN_COLS <= d <= xwideref.MAX_COLS for d in xwideref.COLS)


def test_row_counts_reach_two_reference_shares():
    assert xwideref.ROWS == (1, 2, 31, 32, 33, 127, 128, 129, 300, 1500, 2100)
    assert xwideref.blocks(1500) == 12 and xwideref.shares(12) == 1
    assert xwideref.blocks(2100) == 17 and xwideref.shares(17) == 2
    assert xwideref.shares(15) == 1 and xwideref.shares(16) == 2 and xwideref.shares(31) == 2 and xwideref.shares(32) == 4
    assert xwideref.shares(10 ** 6) == 64
    assert xwideref.tile_pairs(17, 17) == 17 * 17 * 16
    # the product's own rule, where its host code prints it
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_wide_model")
    for rb in (1, 12, 15, 16, 17, 31, 32, 511, 512, 100000):
        out = subprocess.run([exe, "--shares", str(rb)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
        assert out[0] == "shares" and int(out[2]) == xwideref.shares(rb), rb


@pytest.mark.parametrize("gq,gs", [(8, 8), (4, 4), (2, 2), (2, 4), (8, 1)])
def test_the_unit_map_of_any_group_meets_every_query_block_and_share_once(gq, gs):
    """the group shape is a parameter of the map: whatever it is, every (query block, share) has exactly
    one workgroup, the shares are capped by the 8 gs share slots of a launch, and the 8 x 8 group is the map it was"""
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_xwide_model")
    for rb, qb in ((1, 1), (17, 17), (100, 37), (782, 782)):
        out = subprocess.run([exe, "--units", str(gq), str(gs), str(rb), str(qb)], capture_output=True, text=True, timeout=60,
                             check=True).stdout.split("\n")
        n_shares, grid = int(out[0].split()[1]), int(out[1].split()[1])
        assert n_shares == min(xwideref.shares(rb), 8 * gs)
        units = [tuple(int(x) for x in line.split()) for line in out[2:] if line]
        assert len(units) == grid and grid % (8 * gq * gs) == 0
        seen = [(q, s) for _, q, s in units if q < qb]
        assert len(seen) == len(set(seen)) == qb * n_shares and all(s < n_shares for _, s in seen)
        if (gq, gs) == (8, 8):
            old = subprocess.run([os.path.join(ROOT, "clustering_amd", "bin", "test_wide_model"), "--units", str(n_shares), str(qb)],
                                 capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
            assert old[1:] == out[2:] and int(old[0].split()[1]) == grid
        # the workgroups of an XCD (ids = xcd mod 8) that run side by side, 64 at a time, hold gs shares
        side_by_side = [u for u in units if u[0] % 8 == 0][:64]
        assert len({s for _, _, s in side_by_side}) <= gs


@pytest.mark.parametrize("n_cols", [257, 300, 512, 1024])
def test_the_restated_band_is_the_products(n_cols):
    exe = os.path.join(ROOT, "clustering_amd", "bin", "test_xwide_model")
    assert os.path.exists(exe), "__graft_entry__.build() makes it"
    for m in (1e-6, 0.37, 3.57, 8.77, 5.0e4, 2.0e9):
        out = subprocess.run([exe, "--band", str(n_cols), repr(m)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
        assert out[0] == "band" and int(out[1]) == n_cols
        s = xwideref.pick_scale_nn(m)
        sm = float(np.float32(m) * np.float32(s))
        assert 2.0 ** 26 <= sm < 2.0 ** 28
        assert abs(float(out[2]) - s) <= 1e-8 * s   # (printed with nine digits; S is a power of two, the next one is 4 S)
        # (the product rounds its doubles to float and steps one float up)
        assert abs(float(out[3]) - xwideref.guard_e0(sm, n_cols)) <= 3e-7 * float(out[3])
        assert abs(float(out[4]) - xwideref.guard_kappa(n_cols)) <= 3e-7 * float(out[4])


def test_band_constants_at_the_three_widths():
    """e0 / (S M) and kappa as DESIGN.md 4.31 states them (the flush terms add 5e-6 of S M at most at S M >= 2^26)"""
    for n_cols, e0_rel, kappa in ((256, 9.2e-5, 4.8e-5), (512, 1.78e-4, 9.6e-5), (1024, 3.51e-4, 1.91e-4)):
        sm = 2.0 ** 27
        assert abs(xwideref.guard_e0(sm, n_cols) / sm - e0_rel) <= 0.02 * e0_rel, n_cols
        assert abs(xwideref.guard_kappa(n_cols) - kappa) <= 0.02 * kappa, n_cols


@pytest.mark.parametrize("n_cols", xwideref.BAND_COLS)
def test_the_exact_path_cap_is_a_small_share_of_the_pairs(n_cols):
    c, radii, bound, pairs = xwideref.band_case(n_cols)
    assert c.shape == (xwideref.BAND_ROWS, n_cols) and pairs == 1500 * 1499
    d2 = xwideref.pair_d2(c)[~np.eye(len(c), dtype=bool)]
    for r, q in zip(radii, (0.25, 0.05)):
        assert abs(float((d2 < r * r).mean()) - q) < 1e-3, "the radii sit at the quantiles of the pair distances"
    print(f"D={n_cols}: at most {bound} of {pairs} ordered pairs = {100.0 * bound / pairs:.3f} % can reach the exact path")
    assert 0 < bound < 0.02 * pairs
