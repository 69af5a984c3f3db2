"""GPU: the neighbour blocks of a sharded run in the order of the pruned sweep of 257..1024 columns
(density.pack_neighbor_block_xwide / unpack_neighbor_blocks_xwide).  For every shape the segment sweeps
run, each packs its block, the blocks are concatenated and unpacked: the four arrays equal the whole call and the CPU
oracle bit for bit.  Pads hold "none", the payload is the segment's rows by local position of the device's own order, the
header says under which layout the block was packed; a tampered header word of one block makes the unpack write nothing
and the status read 1, the next clean unpack reads 0; a workspace that was never prepared packs under a mark no unpack
accepts; flagged data goes through the reference's row blocks; a block packed at 256 columns is refused.
Cases: tests/xwidegraphref.py, tests/xwidepruneref.py (premises: tests/test_xwide_graph_cases.py)."""
import numpy as np
import pytest

import widesessionref as W
import xwidegraphref as xg
import xwidepruneref as xp

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


def same(got, want, what=""):
    assert (got[0] == want[0]).all(), ("nn_idx", what)
    assert (bits(got[1]) == bits(want[1])).all(), ("nn_d2", what)
    assert (got[2] == want[2]).all(), ("hd_idx", what)
    assert (bits(got[3]) == bits(want[3])).all(), ("hd_d2", what)


def cuda(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def sharded(dens, c, fe, G):
    """the G segment sweeps, each followed by its pack -> (blocks int32 [G, 4, block_rows] on the device, the segment
    results as numpy, the device's order, the coordinates on the device)"""
    import torch
    ct, ft = cuda(c), cuda(fe)
    blocks, parts = [], []
    for g in range(G):
        got = dens.nearest_neighbors_xwide_pruned(ct, ft, g, G)
        blocks.append(dens.pack_neighbor_block_xwide(ct, got[0], got[1], got[2], got[3], g, G))
        parts.append(host(got))
    perm = dens.xwide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    assert sorted(perm.tolist()) == list(range(len(c))), "the order is a permutation of the rows"
    return torch.stack(blocks).contiguous(), parts, perm, ct


def order_hash(perm):
    """the 64-bit hash of the order as the device forms it (dc_mfma_wide.hip wide_order_hash_kernel): the wrap-around sum
    over the positions of a mixed (position, row) word -> (low word, high word)"""
    acc = 0
    mask = (1 << 64) - 1
    for p, row in enumerate(perm.tolist()):
        x = (((p << 32) | row) * 0x9E3779B97F4A7C15) & mask
        x ^= x >> 29
        x = (x * 0xBF58476D1CE4E5B9) & mask
        acc = (acc + (x ^ (x >> 32))) & mask
    return acc & 0xFFFFFFFF, acc >> 32


def check_blocks(blocks, perm, want, G, by_position):
    """every block against the layout the device reports: header, payload by local position (or row block), pads"""
    n = len(perm)
    b = blocks.cpu().numpy().astype(np.uint32)
    rows = xg.block_rows(n, G)
    assert b.shape == (G, 4, rows)
    payload = rows - W.HEADER_ROWS
    none = (n + 1, FLT_MAX_BITS, n + 1, FLT_MAX_BITS)
    h_lo, h_hi = order_hash(perm) if by_position else (0, 0)
    for g in range(G):
        hdr = b[g, 0, payload:]
        assert hdr[0] == (MAGIC | (1 if by_position else 0)) and hdr[1] == n and hdr[3] == G, (g, hdr[:8])
        assert (hdr[2], hdr[4]) == ((128, 1) if by_position else (0, 0)), (g, hdr[:8])
        assert (int(hdr[5]), int(hdr[6])) == (h_lo, h_hi), "the hash of the order the device reports"
        assert (hdr[7:] == 0).all(), (g, hdr)
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


@pytest.mark.parametrize("n_rows", xg.BLOCK_ROWS)
@pytest.mark.parametrize("n_cols", xg.BLOCK_COLS)
def test_blocks_of_every_shape_and_segment_count(dens, n_rows, n_cols):
    c, fe, want = xp.nn_case(n_rows, n_cols)
    ct = cuda(c)
    whole = host(dens.nearest_neighbors_xwide_pruned(ct, cuda(fe)))
    if n_rows > 1:
        assert dens.xwide_pruned_info(ct.device)[0] > 0, "the matrix-core kernel did not answer"
    same(whole, want, "the whole call")
    for G in xg.BLOCK_SEGMENTS:
        blocks, parts, perm, ct = sharded(dens, c, fe, G)
        assert dens.neighbor_block_rows_xwide(n_rows, n_cols, G) == xg.block_rows(n_rows, G) == blocks.shape[2]
        check_blocks(blocks, perm, want, G, by_position=True)
        got = host(dens.unpack_neighbor_blocks_xwide(ct, blocks.view(-1), G))
        assert not dens.xwide_layout_status(ct.device)
        same(got, want, ("the oracle", G))
        same(got, whole, ("the whole call", G))


@pytest.mark.parametrize("word", xg.TAMPERED_WORDS)
def test_a_tampered_header_writes_nothing_and_the_next_clean_unpack_reads_zero(dens, word):
    import torch
    n, d, G = 700, 257, 3
    c, fe, want = xp.nn_case(n, d)
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    rows = xg.block_rows(n, G)
    bad = blocks.clone()
    bad[1, 0, rows - W.HEADER_ROWS + word] += 1      # one word of the header of ONE block
    keep = [torch.full((n,), 7, dtype=t, device=ct.device) for t in (torch.int32, torch.float32, torch.int32, torch.float32)]
    dens.unpack_neighbor_blocks_xwide(ct, bad.view(-1), G, out=tuple(keep), check=False)
    assert dens.xwide_layout_status(ct.device), "the verdict of the refused unpack reads 1"
    assert all(bool((t == 7).all()) for t in keep), "a refused unpack writes nothing"
    with pytest.raises(RuntimeError):
        dens.unpack_neighbor_blocks_xwide(ct, bad.view(-1), G)
    got = host(dens.unpack_neighbor_blocks_xwide(ct, blocks.view(-1), G, out=tuple(keep), check=False))
    assert not dens.xwide_layout_status(ct.device), "the next clean unpack reads 0"
    same(got, want)


def test_a_workspace_that_was_never_prepared_packs_under_the_unaccepted_mark(dens):
    """a zeroed workspace of the shape: no flag, no signed order -- the pack writes "none" under a mark no unpack accepts,
    and the unpack in that workspace refuses whatever it is given"""
    import ctypes as C
    import torch
    from clustering_amd import capi
    n, d, G = 300, 401, 2
    c, fe, want = xp.nn_case(n, d)
    ct = cuda(c)
    need = int(capi.lib.dc_hip_xwide_pruned_workspace_bytes(n, d, 1))
    ws = torch.zeros(need, dtype=torch.uint8, device=ct.device)
    rows = xg.block_rows(n, G)
    res = [cuda(want[0].astype(np.int32), np.int32), cuda(want[1]), cuda(want[2].astype(np.int32), np.int32), cuda(want[3])]
    packed = []
    for g in range(G):
        block = torch.full((4, rows), 5, dtype=torch.int32, device=ct.device)
        rc = capi.lib.dc_hip_neighbors_block_pack_xwide_dev(*[dens._dev(t) for t in res], n, d, g, G, dens._dev(ws), need,
                                                            dens._dev(block), dens._stream_ptr())
        capi.check(rc, "dc_hip_neighbors_block_pack_xwide_dev")
        b = block.cpu().numpy().astype(np.uint32)
        payload = rows - W.HEADER_ROWS
        assert b[0, payload] == xg.NO_ORDER_MARK and b[0, payload + 1] == n and b[0, payload + 3] == G
        assert (b[0, :payload] == n + 1).all() and (b[1, :payload] == FLT_MAX_BITS).all(), "nothing is packed"
        assert (b[2, :payload] == n + 1).all() and (b[3] == FLT_MAX_BITS).all()
        packed.append(block)
    keep = [torch.full((n,), 7, dtype=t, device=ct.device) for t in (torch.int32, torch.float32, torch.int32, torch.float32)]
    blocks = torch.stack(packed).contiguous()
    rc = capi.lib.dc_hip_neighbors_block_unpack_xwide_dev(dens._dev(blocks), n, d, G, dens._dev(ws), need,
                                                          *[dens._dev(t) for t in keep], dens._stream_ptr())
    capi.check(rc, "dc_hip_neighbors_block_unpack_xwide_dev")
    bad = C.c_int(0)
    capi.check(capi.lib.dc_hip_xwide_layout_status_dev(dens._dev(ws), C.byref(bad), dens._stream_ptr()))
    assert bad.value == 1 and all(bool((t == 7).all()) for t in keep), "refused: nothing is written"
    # ... and such blocks are refused by a workspace that does hold the order
    good, _, _, ct = sharded(dens, c, fe, G)
    dens.unpack_neighbor_blocks_xwide(ct, blocks.view(-1), G, out=tuple(keep), check=False)
    assert dens.xwide_layout_status(ct.device) and all(bool((t == 7).all()) for t in keep)
    same(host(dens.unpack_neighbor_blocks_xwide(ct, good.view(-1), G)), want)


@pytest.mark.parametrize("G", [2, 3, 5])
@pytest.mark.parametrize("case,n_cols", [("nan cell", 300), ("nan free energy", 401)])
def test_flagged_data_goes_through_row_blocks(dens, case, n_cols, G):
    c, fe, want = xg.nan_cell_case(n_cols) if case == "nan cell" else xg.nan_fe_case(n_cols)
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    assert dens.xwide_pruned_info(ct.device) == (0, 0, 0), "the direct kernel answered"
    for g in range(G):      # the segment call answered for the row block, "none" elsewhere
        lo, hi = W.row_block(len(c), g, G)
        mine = np.zeros(len(c), dtype=bool)
        mine[lo:hi] = True
        assert (parts[g][0][~mine] == len(c) + 1).all() and (parts[g][0][mine] == want[0][mine]).all()
    check_blocks(blocks, perm, want, G, by_position=False)
    got = host(dens.unpack_neighbor_blocks_xwide(ct, blocks.view(-1), G))
    same(got, want, case)
    # ... and clean data in the same workspace packs by position again
    c, fe, want = xp.nn_case(300, n_cols)
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    check_blocks(blocks, perm, want, G, by_position=True)
    same(host(dens.unpack_neighbor_blocks_xwide(ct, blocks.view(-1), G)), want)


def test_a_block_packed_at_256_columns_is_refused(dens, oracle):
    """the same rows, the same segments, one column fewer: packed through the calls of 65..256 columns in their workspace.
    The header carries the layout -- shape, deal, the hash of the order -- and the two orders differ."""
    import torch
    n, G = 300, 2
    c, fe, want = xp.nn_case(n, 257)
    narrow = np.ascontiguousarray(xp.stretched(n, 256, seed=11))
    ct, ft = cuda(narrow), cuda(fe)
    packed = []
    for g in range(G):
        got = dens.nearest_neighbors_wide_pruned(ct, ft, g, G)
        packed.append(dens.pack_neighbor_block_wide(ct, got[0], got[1], got[2], got[3], g, G))
    perm_256 = dens.wide_pruned_order(ct.device).cpu().numpy().astype(np.int64)
    foreign = torch.stack(packed).contiguous()
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    assert foreign.shape == blocks.shape and not np.array_equal(perm, perm_256), "the premise: the same shape, another order"
    keep = [torch.full((n,), 7, dtype=t, device=ct.device) for t in (torch.int32, torch.float32, torch.int32, torch.float32)]
    dens.unpack_neighbor_blocks_xwide(ct, foreign.view(-1), G, out=tuple(keep), check=False)
    assert dens.xwide_layout_status(ct.device) and all(bool((t == 7).all()) for t in keep), "refused: nothing is written"
    mixed = blocks.clone()
    mixed[1] = foreign[1]
    with pytest.raises(RuntimeError):
        dens.unpack_neighbor_blocks_xwide(ct, mixed.view(-1), G)
    same(host(dens.unpack_neighbor_blocks_xwide(ct, blocks.view(-1), G)), want)
    # ... and the calls of the other family refuse these widths before they touch anything
    res = dens.nearest_neighbors_xwide_pruned(ct, cuda(fe), 0, G)
    with pytest.raises(Exception, match="65..256"):
        dens.pack_neighbor_block_wide(ct, res[0], res[1], res[2], res[3], 0, G)


def test_a_tie_between_duplicate_rows_across_the_boundary_of_blocks_0_and_1_goes_to_the_lower_row(dens, oracle):
    c, fe, (a, p, m) = xg.duplicate_tie_case()
    want = oracle.nearest_neighbors(c, fe)
    G = xg.DUPLICATE_SEGMENTS
    blocks, parts, perm, ct = sharded(dens, c, fe, G)
    pos = {int(r): k for k, r in enumerate(perm)}
    assert (pos[p], pos[m]) == (127, 128) and pos[a] // 128 == 1, "the premise, from the device's order"
    got = host(dens.unpack_neighbor_blocks_xwide(ct, blocks.view(-1), G))
    assert int(got[0][a]) == p and int(got[2][a]) == p and got[1][a] == 9.0 and got[3][a] == 9.0
    assert int(got[0][p]) == m and int(got[0][m]) == p and got[1][p] == 0.0
    same(got, want)
    check_blocks(blocks, perm, want, G, by_position=True)
