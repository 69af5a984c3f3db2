"""Without a GPU: the cases of tests/test_gpu_wide_blocks.py and tests/test_gpu_wide_session.py are built and their premises
checked on the CPU (tests/widesessionref.py): a segment that owns no block of the order, a ragged last block, the ties
between rows -- near-duplicates and exact duplicates -- in blocks of different segments that must go to the lowest row, a flagged case and a NaN free energy; the
session cases cover 0 rows, 65 / 100 / 256 columns, 2 / 3 / 5 devices, both neighbour merges and every poison."""
import os
import subprocess
import sys

import numpy as np

import widesessionref as W


def test_the_helper_needs_neither_torch_nor_a_gpu():
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import widesessionref; "
            "assert 'torch' not in sys.modules, 'widesessionref imports torch'") % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_block_case_premises(oracle):
    assert W.check_block_case_premises() == 6


def test_session_case_premises(probe, oracle):
    assert W.check_session_case_premises(probe, oracle) == len(W.ONE_DEVICE) + len(W.MULTI) + len(W.NARROW_AND_BEYOND) + 1


def test_the_block_row_formula_by_hand():
    """values known by hand: one row is one block of 128 positions; 300 rows in 2 segments: blocks 0 and 2 = 256 positions
    against a row block of 150; 1500 rows in 64 segments: one block each against the last row block of 1500 - 63 * 23 = 51"""
    assert W.block_rows(1, 1) == 128 + 32 and W.block_rows(1, 64) == 128 + 32
    assert W.block_rows(300, 2) == 256 + 32 and W.block_rows(300, 1) == 384 + 32
    assert W.block_rows(1500, 64) == 128 + 32 and W.row_block(1500, 63, 64) == (1449, 1500)
    assert W.block_rows(2 ** 20 + 1, 1) == 2 ** 20 + 128 + 32
    assert W.block_rows(0, 3) == 0 and W.block_rows(10, 0) == 0
    # 129 rows in 2 segments: block 0 (128) and block 1 (1 row) against the row blocks 64 and 65
    assert W.block_rows(129, 2) == 128 + 32 and W.row_block(129, 1, 2) == (64, 129)


def test_local_positions_follow_the_deal():
    """segment g owns the blocks g, g + G, ...; its local block k starts at local position 128 k"""
    n, G = 700, 3      # 6 blocks, the last of 60 rows
    assert W.segment_positions(n, 2, G).tolist() == list(range(256, 384)) + list(range(640, 700))
    assert W.local_positions(n, 2, G).tolist() == list(range(128)) + list(range(128, 188))
    assert len(W.segment_positions(300, 4, 5)) == 0
    assert np.array_equal(W.segment_positions(n, 0, 1), np.arange(n))
