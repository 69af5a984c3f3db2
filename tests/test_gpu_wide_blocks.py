"""GPU: the neighbour blocks of a sharded run in the order of the pruned wide sweep (density.pack_neighbor_block_wide /
unpack_neighbor_blocks_wide, 65..256 columns).  For every shape the segment sweeps run, each packs its block, the blocks
are concatenated and unpacked: the four arrays equal the whole call and the CPU oracle bit for bit, and the per-row
minimum of the packed (d2 bits << 32 | index) words of the segment results.  Pads hold "none", the payload is the
segment's rows by local position of the device's own order, the header says under which layout the block was packed;
a tampered header of one block makes the unpack write nothing and the status read 1, the next clean unpack reads 0;
flagged data goes through the reference's row blocks.  Cases: tests/widesessionref.py (premises:
tests/test_wide_session_cases.py)."""
import numpy as np
import pytest

import widepruneref as pr
import widennpruneref as nnref
import widesessionref as W

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max
FLT_MAX_BITS = int(np.array([FLT_MAX], dtype=np.float32).view(np.uint32)[0])
MAGIC = 0x6E6E5700


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


def host(got):
    return u64(got[0]), got[1].cpu().numpy(), u64(got[2]), got[3].cpu().numpy()


def words(idx, d2):
    return (bits(d2).astype(np.uint64) << np.uint64(32)) | np.asarray(idx, dtype=np.uint64)


def same(got, want, what=""):
    assert (got[0] == want[0]).all(), ("nn_idx", what)
    assert (bits(got[1]) == bits(want[1])).all(), ("nn_d2", what)
    assert (got[2] == want[2]).all(), ("hd_idx", what)
    assert (bits(got[3]) == bits(want[3])).all(), ("hd_d2", what)


def sharded(dens, c, fe, G):
    """the G segment sweeps, each followed by its pack -> (blocks int32 [G, 4, block_rows] on the device, the segment
    results as numpy, the device's order, the coordinates on the device)"""
    import torch
    ct = torch.from_numpy(c).cuda()
    ft = torch.from_numpy(np.ascontiguousarray(fe, dtype=np.float32)).cuda()
    blocks, parts = [], []
    for g in range(G):
        got = dens.nearest_neighbors_wide_pruned(ct, ft, g, G)
        blocks.append(dens.pack_neighbor_block_wide(ct, got[0], got[1], got[2], got[3], g, G))
        parts.append(host(got))
    perm = dens.wide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    return torch.stack(blocks).contiguous(), parts, perm, ct


def check_blocks(blocks, perm, want, G, by_position):
    """every block against the layout: header, payload by local position (or row block), pads"""
    n = len(perm)
    b = blocks.cpu().numpy().astype(np.uint32)
    rows = W.block_rows(n, G)
    assert b.shape == (G, 4, rows)
    payload = rows - W.HEADER_ROWS
    none = (n + 1, FLT_MAX_BITS, n + 1, FLT_MAX_BITS)
    for g in range(G):
        hdr = b[g, 0, payload:]
        assert hdr[0] == (MAGIC | (1 if by_position else 0)) and hdr[1] == n and hdr[3] == G, (g, hdr[:8])
        assert (hdr[2], hdr[4]) == ((128, 1) if by_position else (0, 0)), (g, hdr[:8])
        assert (hdr[5:7] == b[0, 0, payload + 5:payload + 7]).all() and (hdr[7:] == 0).all(), (g, hdr)
        if not by_position:
            assert hdr[5] == 0 and hdr[6] == 0
        for k in (1, 2, 3):
            assert (b[g, k, payload:] == none[k]).all(), "the header entries of the other planes hold none"
        if by_position:
            rows_of, local = perm[W.segment_positions(n, g, G)], W.local_positions(n, g, G)
        else:
            lo, hi = W.row_block(n, g, G)
            rows_of, local = np.arange(lo, hi), np.arange(hi - lo)
        pad = np.ones(payload, dtype=bool)
        pad[local] = False
        for k in range(4):
            expect = want[k][rows_of].astype(np.uint32) if k % 2 == 0 else bits(want[k][rows_of])
            assert (b[g, k, local] == expect).all(), ("payload", g, k)
            assert (b[g, k, :payload][pad] == none[k]).all(), ("pads", g, k)


@pytest.mark.parametrize("n_rows", W.BLOCK_ROWS)
@pytest.mark.parametrize("n_cols", W.BLOCK_COLS)
def test_blocks_of_every_shape_and_segment_count(dens, n_rows, n_cols):
    import torch
    c, fe, want = W.stretched_case(n_rows, n_cols)
    ct = torch.from_numpy(c).cuda()
    whole = host(dens.nearest_neighbors_wide_pruned(ct, torch.from_numpy(fe).cuda()))
    same(whole, want, "the whole call")
    for G in W.BLOCK_SEGMENTS:
        blocks, parts, perm, ct = sharded(dens, c, fe, G)
        assert sorted(perm.tolist()) == list(range(n_rows))
        check_blocks(blocks, perm, want, G, by_position=True)
        got = host(dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), G))
        assert not dens.wide_layout_status(ct.device)
        same(got, want, ("the oracle", G))
        same(got, whole, ("the whole call", G))
        nn = np.minimum.reduce([words(p[0], p[1]) for p in parts])
        hd = np.minimum.reduce([words(p[2], p[3]) for p in parts])
        assert (words(got[0], got[1]) == nn).all() and (words(got[2], got[3]) == hd).all(), "the per-row minimum of the packed words"


def test_a_segment_without_a_block_packs_none_everywhere(dens):
    n, d, G = W.NO_BLOCK
    c, fe, want = W.stretched_case(n, d)
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    b = blocks.cpu().numpy().astype(np.uint32)
    payload = W.block_rows(n, G) - W.HEADER_ROWS
    for g in (3, 4):
        assert (b[g, 0, :payload] == n + 1).all() and (b[g, 1, :payload] == FLT_MAX_BITS).all()
        assert (parts[g][0] == n + 1).all() and (parts[g][1] == FLT_MAX).all()
    same(host(dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), G)), want)


def test_a_tie_across_blocks_of_different_segments_goes_to_the_lowest_row(dens, oracle):
    c, fe, (a, p, q) = nnref.cross_block_tie_case()
    want = oracle.nearest_neighbors(c, fe)
    blocks, parts, perm, ct = sharded(dens, c, fe, W.TIE_SEGMENTS)
    pos = {int(r): k for k, r in enumerate(perm)}
    assert [pos[r] // 128 % W.TIE_SEGMENTS for r in (p, a, q)] == [0, 1, 2], "the premise, from the device's order"
    got = host(dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), W.TIE_SEGMENTS))
    assert int(got[0][a]) == q and int(got[2][a]) == q and got[1][a] == 9.0 and got[3][a] == 9.0
    same(got, want)


def test_a_tie_between_duplicate_rows_in_blocks_of_different_segments_goes_to_the_lowest_row(dens, oracle):
    c, fe, (a, p, m) = W.duplicate_tie_case()
    want = oracle.nearest_neighbors(c, fe)
    G = W.DUPLICATE_SEGMENTS
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    pos = {int(r): k for k, r in enumerate(perm)}
    assert (pos[p], pos[m]) == (127, 128) and pos[a] // 128 == 1, "the premise, from the device's order"
    got = host(dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), G))
    assert int(got[0][a]) == p and int(got[2][a]) == p and got[1][a] == 9.0 and got[3][a] == 9.0
    assert int(got[0][p]) == m and int(got[0][m]) == p and got[1][p] == 0.0
    same(got, want)
    check_blocks(blocks, perm, want, G, by_position=True)


@pytest.mark.parametrize("word", [0, 1, 3, 5, 6])
def test_a_tampered_header_writes_nothing_and_the_next_clean_unpack_reads_zero(dens, word):
    import torch
    n, d, G = 700, 100, 3
    c, fe, want = W.stretched_case(n, d)
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    rows = W.block_rows(n, G)
    bad = blocks.clone()
    bad[1, 0, rows - W.HEADER_ROWS + word] += 1      # one word of the header of ONE block
    keep = [torch.full((n,), 7, dtype=t, device=ct.device) for t in (torch.int32, torch.float32, torch.int32, torch.float32)]
    dens.unpack_neighbor_blocks_wide(ct, bad.view(-1), G, out=tuple(keep), check=False)
    assert dens.wide_layout_status(ct.device), "the verdict of the refused unpack"
    assert all(bool((t == 7).all()) for t in keep), "a refused unpack writes nothing"
    with pytest.raises(RuntimeError):
        dens.unpack_neighbor_blocks_wide(ct, bad.view(-1), G)
    got = host(dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), G, out=tuple(keep), check=False))
    assert not dens.wide_layout_status(ct.device), "the next clean unpack reads 0"
    same(got, want)


@pytest.mark.parametrize("G", [2, 3, 5])
@pytest.mark.parametrize("case", ["nan cell", "nan free energy"])
def test_flagged_data_goes_through_row_blocks(dens, case, G):
    c, fe, want = W.flagged_case() if case == "nan cell" else W.nan_fe_case()
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    assert dens.wide_pruned_info(ct.device) == (0, 0, 0), "the direct kernel answered"
    for g in range(G):      # the segment call answered for the row block, "none" elsewhere
        lo, hi = W.row_block(len(c), g, G)
        mine = np.zeros(len(c), dtype=bool)
        mine[lo:hi] = True
        assert (parts[g][0][~mine] == len(c) + 1).all() and (parts[g][0][mine] == want[0][mine]).all()
    check_blocks(blocks, perm, want, G, by_position=False)
    got = host(dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), G))
    same(got, want, case)
    # ... and clean data in the same workspace packs by position again
    c, fe, want = W.stretched_case(300, 100)
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    check_blocks(blocks, perm, want, G, by_position=True)
    same(host(dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), G)), want)


def test_blocks_packed_by_position_are_refused_in_a_workspace_of_flagged_data(dens):
    """the unpack holds the blocks to the layout of its OWN workspace: blocks packed by position, then a sweep of flagged
    data in that workspace (row blocks): nothing is scattered"""
    import torch
    n, d, G = 300, 100, 2
    c, fe, want = W.stretched_case(n, d)
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    cf, fef, _ = W.flagged_case()
    dens.nearest_neighbors_wide_pruned(torch.from_numpy(cf).cuda(), torch.from_numpy(fef).cuda(), 0, G)
    keep = [torch.full((n,), 7, dtype=t, device=ct.device) for t in (torch.int32, torch.float32, torch.int32, torch.float32)]
    dens.unpack_neighbor_blocks_wide(ct, blocks.view(-1), G, out=tuple(keep), check=False)
    assert dens.wide_layout_status(ct.device) and all(bool((t == 7).all()) for t in keep)
