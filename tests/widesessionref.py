"""Cases, formulas and the runner of the tests of the WIDE sessions and of the neighbour blocks in the order of the pruned
wide sweep (65..256 columns): tests/test_wide_session_cases.py checks the premises of the cases on the CPU
with a numpy cell order (widepruneref.cell_order), tests/test_gpu_wide_blocks.py and tests/test_gpu_wide_session.py run them
on the device.  The referees are those of tests/sessionref.py (the probe's canonical d2 matrix, the oracle's free energies
and sigma2) and the CPU oracle itself; importing this module needs neither a GPU nor torch."""
import functools

import numpy as np

import sessionref as S
import widepruneref as pr
import widennpruneref as nnref

F32 = np.float32
BLOCK = pr.BLOCK
HEADER_ROWS = 32
FLT_MAX = np.finfo(np.float32).max

# the table of the block-row formula (tests/test_capi_wide_session.py) and the shapes of the block tests
TABLE_ROWS = (1, 127, 128, 129, 300, 1500, 2 ** 20 + 1)
TABLE_SEGMENTS = (1, 2, 3, 5, 8, 64)
BLOCK_COLS = (65, 100, 256)
BLOCK_ROWS = (1, 2, 129, 300, 700, 1500)
BLOCK_SEGMENTS = (2, 3, 5, 8)


def row_block(n_rows, segment, n_segments):
    """the reference's partition: n_rows // n_segments rows each, the last rank takes the remainder -> (lo, hi)"""
    rng = n_rows // n_segments
    return segment * rng, (n_rows if segment == n_segments - 1 else (segment + 1) * rng)


def block_rows(n_rows, n_segments):
    """dc_hip_neighbors_block_rows_wide at 65..256 columns: the larger of the largest segment in positions (segment 0 owns
    ceil(blocks / G) blocks of 128) and the largest row block (the last), plus the 32 header entries"""
    if n_rows == 0 or n_segments == 0:
        return 0
    most = -(-pr.n_blocks(n_rows) // n_segments)
    lo, hi = row_block(n_rows, n_segments - 1, n_segments)
    return max(most * BLOCK, hi - lo) + HEADER_ROWS


def segment_positions(n_rows, segment, n_segments):
    """the positions of the order a segment owns, by local position"""
    out = [np.arange(BLOCK * b, min(BLOCK * (b + 1), n_rows)) for b in pr.segment_blocks(n_rows, segment, n_segments)]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def local_positions(n_rows, segment, n_segments):
    """... and where each of them lies in the segment's block: local block k of the segment starts at 128 k"""
    out = [BLOCK * k + np.arange(min(BLOCK, n_rows - BLOCK * b)) for k, b in enumerate(pr.segment_blocks(n_rows, segment, n_segments))]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


# ---- the cases of the block tests ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stretched_case(n_rows, n_cols):
    """(coords, fe, the oracle's neighbours) of widennpruneref.stretched_case, computed once per shape"""
    return nnref.stretched_case(n_rows, n_cols)


NO_BLOCK = (300, 100, 5)      # rows, columns, segments: 3 blocks of the order, segments 3 and 4 own none
RAGGED = (300, 100, 2)        # the last block holds 44 rows, and segment 0 (blocks 0 and 2) owns it
TIE_SEGMENTS = 3              # widennpruneref.cross_block_tie_case: p, a and q lie in blocks 0, 1, 2 = segments 0, 1, 2
FLAW = (131, 7)               # the cell of the flagged case that holds a NaN
DUPLICATE_SEGMENTS = 2        # duplicate_tie_case: the duplicates close block 0 (segment 0) and open block 1 (segment 1)


@functools.lru_cache(maxsize=None)
def duplicate_tie_case():
    """-> (coords, fe, (a, p, m)): widennpruneref.cross_block_tie_case with row m of the middle group made an exact copy
    of p (free energy included) and q moved out of the tie.  p and m share a cell of the order, which sorts them by row:
    p, the lower row, is the last position of block 0 and m the first of block 1, where a lies too.  d2(a, p) = d2(a, m) =
    9 in every summation order, every other row is further away, and fe[p] = fe[m] < fe[a]: nn and hd of a are p, the
    lower row of two duplicates that sit in blocks of different segments."""
    c, fe, (a, p, q) = nnref.cross_block_tie_case()
    c, fe = c.copy(), fe.copy()
    m = 376
    assert m % 3 == 1 and m != a and m > p, "a row of the middle group behind p"
    c[m], fe[m] = c[p], fe[p]
    c[q, 0] = F32(3.5)
    return np.ascontiguousarray(c), np.ascontiguousarray(fe), (a, p, m)


@functools.lru_cache(maxsize=None)
def flagged_case(n_rows=300, n_cols=100):
    """(coords with one NaN cell, fe, the oracle's neighbours): the statistics pass flags the data, the direct kernel
    answers on the reference's row blocks"""
    from oracle.oracle import Oracle
    c, fe, _ = stretched_case(n_rows, n_cols)
    c = c.copy()
    c[FLAW] = np.nan
    return c, fe, Oracle().nearest_neighbors(c, fe)


@functools.lru_cache(maxsize=None)
def nan_fe_case(n_rows=300, n_cols=100):
    """(coords, fe with NaN among them, the oracle's neighbours): a NaN free energy flags the data of a neighbour call"""
    import fe_families
    from oracle.oracle import Oracle
    o = Oracle()
    c, _, _ = stretched_case(n_rows, n_cols)
    pops = o.populations(c, [nnref.std_radius(n_cols)])[0]
    fe = fe_families.make("nan", c, pops)
    return c, fe, o.nearest_neighbors(c, fe)


def check_block_case_premises():
    """the premises of the block cases under the numpy cell order -> number of cases checked"""
    # a segment that owns no block, a ragged last block
    n, d, G = NO_BLOCK
    assert pr.n_blocks(n) == 3 and [len(segment_positions(n, g, G)) for g in range(G)] == [128, 128, 44, 0, 0]
    assert block_rows(n, G) == 128 + HEADER_ROWS and row_block(n, G - 1, G) == (240, 300)
    n, d, G = RAGGED
    assert n % BLOCK == 44 and list(pr.segment_blocks(n, 0, G)) == [0, 2] and len(segment_positions(n, 0, G)) == 128 + 44
    assert local_positions(n, 0, G).tolist() == list(range(128)) + list(range(128, 172))
    # the tie: p closes block 0, a lies in block 1, q opens block 2; d2(a, p) == d2(a, q) == 9 and q < p
    c, fe, (a, p, q) = nnref.cross_block_tie_case()
    pos = {int(r): k for k, r in enumerate(pr.cell_order(c))}
    blocks = [pos[r] // BLOCK for r in (p, a, q)]
    assert blocks == [0, 1, 2] and [b % TIE_SEGMENTS for b in blocks] == [0, 1, 2], "the three rows sit in blocks of three segments"
    d2 = lambda i, j: float(((c[i].astype(np.float64) - c[j].astype(np.float64)) ** 2).sum())
    assert d2(a, p) == 9.0 == d2(a, q) and q < a < p and fe[p] == fe[q] < fe[a]
    others = np.delete(np.arange(len(c)), [a, p, q])
    assert ((c[others].astype(np.float64) - c[a].astype(np.float64)) ** 2).sum(axis=1).min() > 9.0
    # the duplicates: p closes block 0, its copy m opens block 1; a ties between them and must answer p, the lower row
    from oracle.oracle import Oracle
    c, fe, (a, p, m) = duplicate_tie_case()
    pos = {int(r): k for k, r in enumerate(pr.cell_order(c))}
    assert (pos[p], pos[m]) == (BLOCK - 1, BLOCK) and pos[a] // BLOCK == 1 and p < m
    assert [pos[r] // BLOCK % DUPLICATE_SEGMENTS for r in (p, m)] == [0, 1], "the duplicates sit in blocks of different segments"
    assert (c[p] == c[m]).all() and fe[p] == fe[m] < fe[a] and d2_of(c, a, p) == 9.0 == d2_of(c, a, m)
    others = np.delete(np.arange(len(c)), [a, p, m])
    assert ((c[others].astype(np.float64) - c[a].astype(np.float64)) ** 2).sum(axis=1).min() > 9.0
    want = Oracle().nearest_neighbors(c, fe)
    assert int(want[0][a]) == p and int(want[2][a]) == p and int(want[0][p]) == m and int(want[0][m]) == p
    # the flagged cases
    from prunedref import self_flagged
    c, fe, want = flagged_case()
    assert self_flagged(c) and not self_flagged(stretched_case(300, 100)[0]) and np.isnan(c[FLAW])
    c, fe, want = nan_fe_case()
    assert np.isnan(fe).any() and not self_flagged(c)
    assert (want[2][np.isnan(fe)] == len(c) + 1).all(), "a NaN free energy has no lower neighbour"
    # every shape of the block tests: the blocks of all segments hold every position once, inside the payload
    for n in BLOCK_ROWS:
        for G in BLOCK_SEGMENTS:
            seen = np.concatenate([segment_positions(n, g, G) for g in range(G)])
            assert sorted(seen.tolist()) == list(range(n))
            for g in range(G):
                loc = local_positions(n, g, G)
                assert len(loc) == len(segment_positions(n, g, G)) and (len(loc) == 0 or loc.max() < block_rows(n, G) - HEADER_ROWS)
                lo, hi = row_block(n, g, G)
                assert hi - lo <= block_rows(n, G) - HEADER_ROWS
    assert any(G > pr.n_blocks(n) for n in BLOCK_ROWS for G in BLOCK_SEGMENTS) and any(n % BLOCK for n in BLOCK_ROWS)
    return 6


def d2_of(c, i, j):
    return float(((c[i].astype(np.float64) - c[j].astype(np.float64)) ** 2).sum())


# ---- the cases of the session tests ---------------------------------------------------------------------------------------
# one device: (n, D, seed, kind)
ONE_DEVICE = [(513, 65, 165, "lattice"), (1500, 100, 1100, "clustered"), (300, 256, 1256, "lattice")]
# several "devices" on one GPU: (n, D, G, neighbour merge, poison), the form of sessionref.MULTI
MULTI = [
    (0, 100, 2, "allgather", None), (1, 65, 3, "allreduce", None), (2, 100, 5, "allgather", None),
    (129, 256, 2, "allreduce", None), (300, 100, 5, "allgather", None), (300, 65, 3, "allgather", "nan"),
    (700, 100, 3, "allreduce", None), (700, 65, 5, "allgather", None), (1500, 100, 2, "allgather", None),
    (1500, 256, 5, "allreduce", None), (1500, 100, 3, "allgather", "inf"), (700, 256, 2, "allreduce", "2e18"),
    (700, 100, 2, "allgather", "6e16"),
]
# one cell replaced: NaN, inf and 2e18 (|x - mean|^2 = 4e36, beyond the 1e36 of the wide sweeps' statistics pass) flag the
# data; 6e16 flags the sweeps of at most 64 columns (sessionref.POISON) and NOT the wide ones, which answer themselves
POISON = {"nan": np.nan, "inf": np.inf, "2e18": 2.0e18, "6e16": 6.0e16}
NORM_LIMIT = 1.0e36
NARROW_AND_BEYOND = [(700, 10, 31), (300, 300, 32)]     # (n, D, seed): the flag changes nothing outside 65..256 columns
DEFAULT_CASE = (700, 100, 41)                            # ... and a default session of wide rows stays as it is


def one_data(case):
    n, D, seed, kind = case
    return S.data(kind, n, D, seed)


def wide_flagged(c):
    """True where the statistics pass of a wide sweep flags the data (dc_mfma_wide_kernels.hpp wide_rowstats_kernel): a row
    whose |x - mean|^2 is not finite or beyond 1e36.  Formed in float64 here: the cases stay orders of magnitude away from
    the limit on either side."""
    c = np.asarray(c, dtype=np.float64)
    if c.size == 0:
        return False
    with np.errstate(invalid="ignore", over="ignore"):
        mean = c.sum(axis=0) / len(c)
        mean = np.where(np.isfinite(mean), mean, 0.0)
        nrm = ((c - mean) ** 2).sum(axis=1)
        return bool((~(nrm <= NORM_LIMIT)).any())


def multi_data(case):
    """-> (coords, coords without the poisoned cell); the cell is sessionref.data's"""
    n, D, G, merge, poison = case
    kind = "clustered" if D == 100 else "lattice"
    clean = S.data(kind, n, D, 700 + D + n)
    c = clean.copy()
    if poison is not None:
        c[(n // 2 + 1) % n, min(4, D - 1)] = POISON[poison]
    return np.ascontiguousarray(c), clean


def multi_ref(probe, oracle, case):
    """-> (Ref of the case with `flagged` by the WIDE sweeps' rule, the radii of the unpoisoned data)"""
    c, clean = multi_data(case)
    ref = S.Ref(probe, oracle, c)
    ref.flagged = wide_flagged(c)
    return ref, S.radii_of(ref if case[4] is None else S.Ref(probe, oracle, clean))


def check_session_case_premises(probe, oracle):
    """the premises of the session cases on the referee's data -> number of cases checked"""
    from prunedref import self_flagged
    count = 0
    for case in ONE_DEVICE:
        n, D, seed, kind = case
        ref = S.Ref(probe, oracle, one_data(case))
        assert 65 <= D <= 256 and n <= 1500 and not ref.flagged
        R = S.radii_of(ref)
        assert len(R["multi9"]) == 9 and len(R["multi3"]) == 3 and len(R["one"]) == 1
        if n >= 500:
            assert 0 < len(ref.pairs(R["r2"]["above"])) < 400000, case
        count += 1
    seen = {"G": set(), "D": set(), "merge": set(), "poison": set(), "n": set()}
    for case in MULTI:
        n, D, G, merge, poison = case
        c, clean = multi_data(case)
        assert wide_flagged(c) == (poison in ("nan", "inf", "2e18")) and not wide_flagged(clean), S.multi_id(case)
        assert self_flagged(c) == (poison is not None), "6e16: flagged below 65 columns only"
        assert 65 <= D <= 256 and n <= 1500 and G <= 5
        ref, R = multi_ref(probe, oracle, case)
        assert ref.flagged == wide_flagged(c)
        for key, v in zip(("G", "D", "merge", "poison", "n"), (G, D, merge, poison, n)):
            seen[key].add(v)
        count += 1
    assert seen["G"] == {2, 3, 5} and seen["D"] == {65, 100, 256} and seen["merge"] == {"allgather", "allreduce"}
    assert seen["poison"] == {None, "nan", "inf", "2e18", "6e16"} and seen["n"] >= {0, 1, 2, 129, 300, 1500}
    assert any(G > pr.n_blocks(n) for n, D, G, m, p in MULTI if n > 0), "a device without a block of the order"
    for n, D, seed in NARROW_AND_BEYOND + [DEFAULT_CASE]:
        assert (not 65 <= D <= 256) or (n, D, seed) == DEFAULT_CASE
        ref = S.Ref(probe, oracle, S.data("lattice", n, D, seed))
        assert not ref.flagged
        S.radii_of(ref)
        count += 1
    return count


class WideFlow(S.Flow):
    """sessionref.Flow over a session opened with wide=True: the same steps held to the same referee; who answered is
    the rule of the wide sessions -- inside 65..256 columns the counters hold the evaluated tile pairs of the pruned wide
    sweeps, more than 0 on unflagged data (populations: with some radius that squares to more than 0) and 0 on flagged
    data and under a NaN free energy; outside those widths the session is a default one (sessionref.Flow.who)"""

    def who(self, kind, step, radii=None, fe=None):
        if not 65 <= self.ref.D <= 256:
            assert not self.s.wide
            return super().who(kind, step, radii=radii, fe=fe)
        assert self.s.wide
        if self.ref.n == 0:
            return
        tiles = self.call(self.s.counters)[0 if kind == "pop" else 1]
        fe_nan = fe is not None and bool(np.isnan(fe).any())
        if self.ref.flagged or fe_nan:
            assert tiles == 0, (self.what, step, "the direct kernel should have answered", tiles)
        elif kind == "pop":
            with np.errstate(invalid="ignore", over="ignore"):
                some = bool((np.array([S.square(r) for r in radii]) > 0).any())
            if some:
                assert tiles > 0, (self.what, step, "the session is not on the wide sweeps: evaluated tiles", tiles, radii)
        else:
            assert tiles > 0, (self.what, step, "the session is not on the wide sweeps: evaluated tiles", tiles)


def open_wide_flow(dens, ref, what, R=None, **session_args):
    S.OPENED[0] += 1
    return WideFlow(dens, ref, dens.Session(ref.c, wide=True, **session_args), what, R=R)
