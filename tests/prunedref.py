"""Cases, referees and plumbing of the pruned self-sweep edge tests (tests/test_gpu_pruned_edges.py, its child processes
and the GPU-free condition test tests/test_pruned_edge_cases.py): data whose d2 are exact in every summation order
(tests/graphref.py), radii whose fl32(r * r) sits at, one float above and one float below a lattice d2, the expected
populations and neighbours from the probe's canonical d2 matrix (tests/crossref.py, with the self-sweep conventions of
include/dc_density.h), and the CPU restatement of which kernel has to answer.  Importing this module needs neither a
GPU nor torch; only Self (the runner) touches the device."""
import ctypes as C

import numpy as np

import fe_families
from crossref import F32, FLT_MAX, bits, expect_nn, expect_pops, gpu, host, same_nn, square
from graphref import INF, NAN, TRANSFORMS, clustered_lattice, lattice, level_of, tie_radii, transformed, with_isolated

WIDTHS = (1, 3, 10, 17, 24, 30, 40, 64)
STATS_LIMIT = F32(5.0e16)   # dc_prep.hpp:25 kStatsLimit
FE_NAMES = ("continuous", "constant", "ties_ulp", "nan")


def nm_for(D):
    """MFMAs per chain of the matrix-core sweeps (dc_mfma_kernels.hpp nm_for): three fp16 pieces per column + 2 slots"""
    return (3 * D + 2 + 15) // 16


def self_flagged(c):
    """True where the ONE statistics pass of a pruned self sweep flags the data (dc_prep.hpp:54-64 and :88,
    stats_kernel: `fin = fabsf(v) <= kStatsLimit; bad |= !fin; ... if (bad) atomicOr(hdr + 1, 1u)`): any element that is
    not finite or beyond 5e16 in magnitude -- element-wise, unlike the cross sweeps' |x - mean|^2 > 1e36
    (crossref.stats_flagged).  The matrix-core kernels then return at once (`if (hdr[1] != 0) return`) and the gated
    exact kernel answers."""
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(np.asarray(c, dtype=np.float32)) <= STATS_LIMIT)).any())


# ---- radii --------------------------------------------------------------------------------------------------------------
def radius_for(r2):
    """a float radius with fl32(r * r) == r2, or None: the library squares its radii, and only some floats are squares
    of a float (near T in [1, 2) every other one at best)"""
    t = F32(r2)
    base = int(np.array([np.sqrt(np.float64(t))], dtype=np.float32).view(np.uint32)[0])
    for r in (base + np.arange(-16, 17, dtype=np.int64)).astype(np.uint32).view(np.float32):
        if square(r) == t:
            return float(r)
    return None


def tie_radii_of(d2, levels=(0, 1, 2), need_above=True):
    """radii at the lowest lattice levels of d2: per level graphref.tie_radii (whose assertions are conditions of the
    case: pairs AT the level, pairs one float below the float above it), each squared radius turned into a radius where
    one exists -> (at, above, below): lists of radii whose squares are the level / the float above / the float below.
    A condition of the case: at least two levels are reached exactly and at least two from one float above
    (need_above=False, one column: the levels are squares of integers, and the float above g^2 is the square of a float
    for no g below 23 -- such data serves the ties AT the radius only)."""
    at, above, below = [], [], []
    for k in levels:
        lo, t, hi = tie_radii(d2, level_of(d2, k))
        for r2, out in ((lo, below), (t, at), (hi, above)):
            r = radius_for(r2)
            if r is not None:
                out.append(r)
    assert len(at) >= 2 and (len(above) >= 2 or not need_above), ("broken tie case: too few reachable radii", at, above, below)
    return at, above, below


def radius_lists(at, above, below, scale=1.0):
    """the calls of a tie case: every tie radius alone, and multi-radius calls of 3, 8 and 11 radii (one launch, a full
    launch, two launches: kMaxRadiiPerLaunch = 8) in UNSORTED order with 0, 1e-30, inf, 1e20, NaN and a repeated radius
    mixed in -> (singles, multis)"""
    ties = at + above + below
    far = float(F32(40.0 * scale))    # beyond the lattice's extent
    up = above or at[1:]
    three = [up[0], at[0], at[-1]]
    eight = [at[-1], 0.0, up[0], INF, at[0], NAN, up[-1], at[0]]
    eleven = [up[-1], 1e-30, at[0], far, NAN, at[-1], 1e20, up[0], at[0], (below or at)[0], 0.0]
    assert len(eight) == 8 and len(eleven) == 11
    return ties, [three, eight, eleven]


# ---- referees: the self-sweep conventions of include/dc_density.h ----------------------------------------------------------
def off_diagonal(d2):
    """the d2 matrix with NaN on the diagonal: a frame is never its own partner (every comparison with NaN is false)"""
    out = np.array(d2, dtype=np.float32, copy=True)
    np.fill_diagonal(out, np.nan)
    return out


def expect_self_pops(d2x, radii, i_from=0, i_to=None):
    """pop_r[i] = 1 + #{ j != i : d2(i, j) < fl32(r * r) } for i in [i_from, i_to), 0 outside"""
    i_to = d2x.shape[0] if i_to is None else i_to
    out = expect_pops(d2x, radii, i_from, i_to)
    out[:, i_from:i_to] += 1
    return out


def expect_self_nn(d2x, fe, i_from=0, i_to=None):
    """nn = lexicographic min over j != i of (d2, j); nn_hd the same over fe[j] < fe[i]; none = (n + 1, FLT_MAX)"""
    return expect_nn(d2x, fe, fe, i_from, i_to)


def nn_tie_share(d2x):
    """share of the queries with two or more candidates at the minimal d2, that d2 being positive"""
    with np.errstate(invalid="ignore"):
        m = np.nanmin(d2x, axis=1)
        return float((((d2x == m[:, None]).sum(axis=1) >= 2) & (m > 0)).mean())


def fe_set(c, pops, seed=0, names=FE_NAMES):
    """the free energies of a case's neighbour checks: fe_families by name + those of the case's own populations"""
    out = [(name, fe_families.make(name, c, pops, seed=seed)) for name in names]
    out.append(("own populations", fe_families.make("pops", c, pops, seed=seed)))
    return out


# ---- tie cases ----------------------------------------------------------------------------------------------------------
def tie_data(D, kind, n, seed, transform):
    """-> (coords, scale): lattice or clustered lattice, under one of graphref.TRANSFORMS (d2 stay exact)"""
    c = (lattice if kind == "lattice" else clustered_lattice)(n, D, seed)
    name, scale, shift = transform
    out, _ = transformed(c, 1.0, scale, shift)
    return out, scale


def tie_plan(reduced=False):
    """(D, kind, n, transform) of the tie cases: every width on the lattice and the clustered lattice by turns, plain
    and under ONE other transform by turns (all four transforms occur twice or more); reduced (the children of the forced forms):
    one transform each, and without one column (whose levels no float above is reached for) and 30 columns (6 MFMAs per
    chain: the same forms as 24 and 40) -- 1, 2, 4, 5, 8 and 13 MFMAs per chain remain"""
    plan = []
    widths = (3, 10, 17, 24, 40, 64) if reduced else WIDTHS
    for k, D in enumerate(widths):
        kind = ("lattice", "clustered")[k % 2]
        n = 1300 if D <= 3 else (2500 if not reduced else 2200)
        turns = [TRANSFORMS[1 + k % 3]] if reduced else [TRANSFORMS[0], TRANSFORMS[1 + k % 3]]
        for t in turns:
            plan.append((D, kind, n, t))
    return plan


def neighbour_ties_required(D):
    """widths 1 and 3: nearly every frame has an exact duplicate -- they serve populations and d2 = 0 ties only"""
    return D >= 10


def check_tie_case(d2x, D):
    """the CPU-side conditions of a tie case beyond tie_radii's own -> (at, above, below) in units of the lattice"""
    if neighbour_ties_required(D):
        share = nn_tie_share(d2x)
        assert share >= 0.10, f"broken tie case: only {share:.3f} of the queries have tied nearest candidates at d2 > 0"
    else:
        assert (d2x == 0).any(), "broken tie case: no duplicates"
    return tie_radii_of(d2x, need_above=D > 1)


# ---- the pruning rule: two sets at a box gap ----------------------------------------------------------------------------------
def gap_sets(D, g, mode, seed=0, rows=200):
    """Two sets of `rows` integer points each, mixed -> (coords, T): T the d2 of the closest cross pairs.
      "plane"   A: col 0 in -3..0, B: col 0 in g..g+3, col 1 in 0..3 for both, other columns 0: box gap g, closest cross
                pairs at exactly g^2
      "beyond"  the same boxes, and B one step up in columns 2..4 where A is 0 (D >= 5): closest cross pairs at g^2 + 3,
                box gap still g -- the plane test must keep the tile pair, the full d2 decides
      "equal"   both sets uniform on {0..3}^2 in columns 0/1 (gap 0: never pruned, one component), apart by g in column 2
    Conditions checked here: cross pairs exist exactly at T and none below."""
    rng = np.random.default_rng(seed + 7 * D + g)
    a = np.zeros((rows, D), dtype=np.float32)
    b = np.zeros((rows, D), dtype=np.float32)
    a[:, 1] = rng.integers(0, 4, rows)
    b[:, 1] = rng.integers(0, 4, rows)
    if mode == "equal":
        a[:, 0] = rng.integers(0, 4, rows)
        b[:, 0] = rng.integers(0, 4, rows)
        b[:, 2] = g
        T = g * g
    else:
        a[:, 0] = -rng.integers(0, 4, rows)
        b[:, 0] = g + rng.integers(0, 4, rows)
        a[:8, 0], a[:8, 1] = 0, np.arange(8) % 4    # the facing edges are populated on every line of column 1
        b[:8, 0], b[:8, 1] = g, np.arange(8) % 4
        T = g * g
        if mode == "beyond":
            assert D >= 5
            b[:, 2:5] = 1
            T = g * g + 3
    c = np.concatenate([a, b])
    side = np.concatenate([np.zeros(rows, dtype=bool), np.ones(rows, dtype=bool)])
    order = rng.permutation(len(c))
    return np.ascontiguousarray(c[order]), side[order], float(T)


def check_gap_case(d2, side, T):
    cross = d2[np.ix_(~side, side)]
    assert (cross == F32(T)).any() and not (cross < F32(T)).any(), "broken gap case: the closest cross pairs are not at T"


def gap_radii(T, g):
    """radii of a gap case: r2 == T (the closest cross pairs AT the radius: outside), the float above T (inside), the
    plane gap itself, and 1 (far below) -- conditions: both tie radii exist as floats"""
    at, above = radius_for(T), radius_for(np.nextafter(F32(T), F32(np.inf)))
    assert at is not None and above is not None, f"broken gap case: T = {T} is not reachable from both sides"
    return [at, above, float(g), 1.0]


# (g, T) with fl32(r * r) reaching T and the float above it: T = g^2 for the plane case, g^2 + 3 for "beyond"
GAP_PLANE = 23     # 529 and the float above it are squares of floats (checked by gap_radii): no smaller g^2 has both
GAP_BEYOND = 3     # 9 + 3 = 12: both reachable


# ---- the component cut ------------------------------------------------------------------------------------------------------
def cluster_row(D, k, sep, seed, rows=260):
    """k lattice clusters (columns 0/1 in -1..4, graphref.lattice) in a row along column 0 whose BOXES are sep apart:
    cluster j spans [j (5 + sep) - 1, j (5 + sep) + 4] in column 0 (both ends populated)"""
    rng = np.random.default_rng(seed)
    parts = []
    for j in range(k):
        c = lattice(rows, D, seed + j)
        c[:16, 1:] = 0.0                        # the facing edges hold frames equal in every other column
        c[:8, 0], c[8:16, 0] = -1.0, 4.0
        c[:, 0] += j * (5.0 + sep)
        parts.append(c)
    c = np.concatenate(parts)
    return np.ascontiguousarray(c[rng.permutation(len(c))], dtype=np.float32)


def check_cluster_row(c, k, sep):
    x = np.sort(np.unique(c[:, 0]))
    gaps = np.diff(x)
    if sep == 1:
        assert (gaps == 1).all() and len(x) == 6 * k, "broken component case: the clusters do not touch"
        return
    assert (gaps == sep).sum() == k - 1 and (gaps[gaps != sep] == 1).all(), "broken component case: the boxes are not sep apart"


def cluster_grid(D, k, spacing, seed, rows=24):
    """k x k small lattice clusters on a grid in columns 0/1 (more than the 64 component slots for k >= 9)"""
    rng = np.random.default_rng(seed)
    parts = []
    for a in range(k):
        for b in range(k):
            c = rng.integers(0, 3, (rows, D)).astype(np.float32)
            c[:, 0] += a * spacing
            c[:, 1 if D > 1 else 0] += b * spacing
            parts.append(c)
    c = np.concatenate(parts)
    assert c.max() <= 4000.0
    return np.ascontiguousarray(c[rng.permutation(len(c))], dtype=np.float32)


# ---- emptiness and tiny shapes ------------------------------------------------------------------------------------------
def emptiness(D, seed, n=900):
    """a lattice with isolated frames 100 lattice steps from each other and more from the data (graphref.with_isolated:
    hundreds of typical nearest-neighbour distances; the integer d2 stay below 2^24) and free energies under which the
    LAST isolated frame along column 0 has its only lower neighbour at the other end of the data -> (coords, fe, far, low)"""
    c = with_isolated(lattice(n, D, seed), k=7)
    far = int(np.argmax(c[:, 0]))
    low = int(np.argmin(c[:, 0] + 1e-3 * np.arange(len(c))))
    fe = np.full(len(c), 2.0, dtype=np.float32)
    fe[far] = 1.0
    fe[low] = 0.0
    return c, fe, far, low


TINY = (1, 2, 31, 32, 33)


def tiny_sizes():
    """n = 1, 2, 31, 32, 33 and sizes that leave ONE real row in the last tile of 32 and -- the query groups are whole
    tiles, 1 .. 32 of them -- in the last query group whatever the group size: 32 m + 1 for m = 32 and 96"""
    return TINY + (32 * 32 + 1, 32 * 96 + 1)


# ---- the runner ---------------------------------------------------------------------------------------------------------
def same_pops(got, want, what):
    g = host(got).astype(np.int64)
    if not (g == want).all():
        bad = np.argwhere(g != want)
        k, i = bad[0]
        raise AssertionError(f"pops {what}: {len(bad)} entries differ, e.g. radius {k} row {i}: {g[k, i]} != {want[k, i]}")


class Self:
    """one coordinate set on the device with its canonical d2 matrix; every call goes through DC_VARIANT_AUTO (the
    pruned matrix-core sweeps) and is followed by the who-answered check"""

    def __init__(self, dens, probe, c, flagged=False, what=""):
        self.c = np.ascontiguousarray(c, dtype=np.float32)
        self.n, self.D = self.c.shape
        self.what, self.flagged, self.dens = what, flagged, dens
        assert self_flagged(self.c) == flagged, (what, "the case does not reach the path it is meant to")
        self.d2 = probe.pairwise_d2(self.c)
        self.d2x = off_diagonal(self.d2)
        self.t = gpu(self.c)
        self.tiles = {}

    # -- who answered
    def flag_word(self):
        """header word 1 of the self-sweep workspace (bytes 4..7 of the buffer: dc_mfma_kernels.hpp kHdrBytes "word 1:
        non-finite flag"; bit 0 set by stats_kernel, dc_prep.hpp:88, bit 1 by a failed DC_FLAG_STATS_VALID claim, bit 2
        by NaN free energies, dc_prep.hpp:308) -- what every matrix-core kernel tests before it starts"""
        return int(self.dens._workspace(self.t.device).buf[4:8].cpu().numpy().view(np.uint32)[0])

    def answered(self, kind, what, radii=None, fe=None, tiles_sure=True):
        """after a sweep of `kind` ("pop" / "nn"): the pruned matrix-core kernel answered -- flag word 0 and evaluated
        tiles > 0 -- unless the case trips the statistics flag (or hands in a NaN free energy: bit 2), then 0 tiles.
        A population call whose radii all square to 0 or NaN keeps no tile pair (box_gap2 < r2max * 1.0001f is false for
        r2max = 0): flag word 0 and 0 tiles.  tiles_sure=False (a segment of more segments than there are query
        groups for sure): the flag word only."""
        tiles = self.dens.evaluated_tiles(self.t.device)[0 if kind == "pop" else 1]
        word = self.flag_word()
        self.tiles[kind] = tiles
        fe_nan = fe is not None and bool(np.isnan(fe).any())
        if self.flagged or fe_nan:
            assert word != 0 and tiles == 0, (what, "the exact kernel should have answered", word, tiles)
            return
        assert word == 0, (what, "the matrix-core kernel should have answered, flag word", word)
        if not tiles_sure:     # (a segment that may own no query group)
            return
        if kind == "pop":
            with np.errstate(invalid="ignore"):
                some = bool((np.array([square(r) for r in radii]) > 0).any())
            assert (tiles > 0) == some, (what, "evaluated tiles", tiles, "radii", radii)
        elif self.n >= 2:
            assert tiles > 0, (what, "evaluated tiles", tiles)

    def owns_a_group(self, g, n_seg):
        """True where segment g of n_seg owns a query group for sure: the groups are dealt out one by one in turn
        (dc_mfma.hpp seg_owns, kSegBlockGroups = 1) and a group has at most 512 rows (dc_mfma_kernels.hpp:126 kMaxGroupRows = 512, which
        the launchers enforce: dc_mfma.hip `32u * group_tiles > kMaxGroupRows` returns; plan_pop / plan_nn give 4 * tq or tq
        tiles), so there are at least ceil(n / 512) of them; segment 0 always owns the first"""
        return g == 0 or g < -(-self.n // 512)

    # -- populations
    def _abi(self, radii, sel, segment):
        import torch
        from clustering_amd import capi
        rad = np.ascontiguousarray(radii, dtype=np.float32)
        out = torch.empty((rad.size, self.n), dtype=torch.int32, device=self.t.device)
        ws, ws_bytes = self.dens._workspace(self.t.device).get(self.n, self.D, rad.size)
        fn = capi.lib.dc_hip_populations_segment_dev if segment else capi.lib.dc_hip_populations_dev
        rc = fn(C.c_void_p(self.t.data_ptr()), self.n, self.D, rad.ctypes.data_as(C.POINTER(C.c_float)), rad.size,
                sel[0], sel[1], C.c_void_p(out.data_ptr()), ws, ws_bytes, capi.VARIANTS["auto"],
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        capi.check(rc, "dc_hip_populations[_segment]_dev")
        return out

    def pops(self, radii, i_from=0, i_to=None, abi=False):
        """all rows or a row range, through Python (radii sorted on the way) or straight into the C ABI as given"""
        i_to = self.n if i_to is None else i_to
        what = (self.what, "radii", radii, "rows", i_from, i_to, "abi" if abi else "python")
        want = expect_self_pops(self.d2x, radii, i_from, i_to)
        if abi:
            got = self._abi(radii, (i_from, i_to), False)
        else:
            got = self.dens.calculate_populations_partial(self.t, radii, i_from, i_to)
        self.answered("pop", what, radii=radii)
        same_pops(got, want, what)
        return want

    def pop_segments(self, radii, n_seg, abi=False):
        """the segments' partial counts summed"""
        what = (self.what, "radii", radii, n_seg, "segments", "abi" if abi else "python")
        acc = None
        for g in range(n_seg):
            if abi:
                p = self._abi(radii, (g, n_seg), True)
            else:
                p = self.dens.calculate_populations_segment(self.t, radii, g, n_seg)
            self.answered("pop", what + (g,), radii=radii, tiles_sure=self.owns_a_group(g, n_seg))
            acc = p.clone() if acc is None else acc + p
        same_pops(acc, expect_self_pops(self.d2x, radii), what)

    # -- neighbours
    def nn(self, fe, i_from=0, i_to=None, name=""):
        i_to = self.n if i_to is None else i_to
        what = (self.what, "nn", name, i_from, i_to)
        got = self.dens.nearest_neighbors_partial(self.t, gpu(fe), i_from, i_to)
        self.answered("nn", what, fe=fe)
        exp = expect_self_nn(self.d2x, fe, i_from, i_to)
        same_nn(got, exp, what)
        return exp

    def nn_segments(self, fe, n_seg, name=""):
        """the segments merged both ways: (d2 bits << 32 | index) words by minimum, and the dense blocks of the
        all-gather; every row is answered by exactly one segment"""
        import torch
        what = (self.what, "nn", name, n_seg, "segments")
        exp = expect_self_nn(self.d2x, fe)
        fe_t = gpu(fe)
        words, blocks = None, []
        owned = np.zeros(self.n, dtype=np.int64)
        for g in range(n_seg):
            a, b, cc, d = self.dens.nearest_neighbors_segment(self.t, fe_t, g, n_seg)
            self.answered("nn", what + (g,), fe=fe, tiles_sure=self.owns_a_group(g, n_seg))
            blocks.append(self.dens.pack_neighbor_block(self.t, a, b, cc, d, g, n_seg))
            mine = host(b) != FLT_MAX if self.n > 1 else np.ones(1, dtype=bool)
            owned += mine | (exp[1] == FLT_MAX)     # (a row without any partner looks the same in every segment)
            w = self.dens.pack_neighbors(a, b, cc, d)
            words = w if words is None else torch.minimum(words, w)
        assert (owned >= 1).all() and (owned[exp[1] != FLT_MAX] == 1).all(), (what, "every row belongs to one segment")
        same_nn(self.dens.unpack_neighbors(words.contiguous()), exp, what + ("words",))
        same_nn(self.dens.unpack_neighbor_blocks(self.t, torch.stack(blocks).contiguous(), n_seg), exp, what + ("blocks",))

    # -- the whole programme of a tie case
    def tie_programme(self, scale, n_segs=(2, 3, 5), families=FE_NAMES, many_segments=False):
        at, above, below = check_tie_case(self.d2x, self.D)
        above = above or at[1:]
        singles, multis = radius_lists(at, above, below, float(scale))
        n = self.n
        ranges = ((37, n - 45), (n // 3 + 5, n // 3 + 75))     # (start and end inside a tile and inside a query group)
        for r in singles:
            self.pops([r])
        for r in at:    # the strict < at the tie: a radius whose square is the level leaves its pairs out
            t = square(r)
            w = self.pops([r])
            with np.errstate(invalid="ignore"):
                assert (w[0] == 1 + (self.d2x < t).sum(axis=1)).all() and ((self.d2x == t).sum() > 0)
        for radii in multis:
            self.pops(radii)
            self.pops(radii, abi=True)
            for lo, hi in ranges:
                self.pops(radii, lo, hi)
            self.pops(radii, *ranges[0], abi=True)
        for n_seg in n_segs:
            self.pop_segments([above[0]], n_seg)
            self.pop_segments(multis[n_seg % 3], n_seg)
        self.pop_segments(multis[2], 3, abi=True)
        if many_segments:     # more segments than query groups (a group is at least one tile; <= 64 padded components)
            self.pop_segments([at[-1], above[0]], n // 32 + 70)
        pops = expect_self_pops(self.d2x, [above[-1]])[0].astype(np.uint64)
        for name, fe in fe_set(self.c, pops, seed=self.D, names=families):
            self.nn(fe, name=name)
            self.nn(fe, *ranges[0], name=name)
            self.nn_segments(fe, 3, name=name)
        if many_segments:
            self.nn_segments(fe_set(self.c, pops, seed=1, names=("continuous",))[0][1], n // 32 + 70, name="continuous")


def run_ties(dens, probe, plan, log=None, **kw):
    """every tie case of a plan -> per case the evaluated tiles / issued MFMAs of chosen sweeps (for the parents that
    compare the forms)"""
    out = {}
    for D, kind, n, transform in plan:
        c, scale = tie_data(D, kind, n, 100 + D, transform)
        what = f"{kind} D={D} n={n} {transform[0]}"
        s = Self(dens, probe, c, what=what)
        s.tie_programme(scale, many_segments=(D == 10 and transform[0] == "plain"), **kw)
        out[what] = counters(s, scale)
        if log:
            log(what, out[what])
    return out


def counters(s, scale):
    """what the library's own counters say about the forms a case ran in: evaluated tiles and issued MFMAs of a
    one-radius and a five-radius population sweep over all rows, evaluated tiles of a neighbour sweep, the block rows of
    a three-segment neighbour merge and the component count"""
    dev = s.t.device
    r = float(F32(np.sqrt(3.0) * scale))
    s.dens.calculate_populations_partial(s.t, [r])
    one = (s.dens.evaluated_tiles(dev)[0], s.dens.issued_mfmas(dev)[0])
    comps = s.dens.components_info(s.t)["n_components"]
    five = [float(F32(x * scale)) for x in (1.0, 1.5, 1.75, 2.0, 2.25)]
    s.dens.calculate_populations_partial(s.t, five)
    many = (s.dens.evaluated_tiles(dev)[0], s.dens.issued_mfmas(dev)[0])
    s.dens.nearest_neighbors_partial(s.t, gpu(np.zeros(s.n, dtype=np.float32)))
    nn = (s.dens.evaluated_tiles(dev)[1], s.dens.issued_mfmas(dev)[1])
    return {"nm": nm_for(s.D), "one": one, "five": many, "nn": nn, "components": comps,
            "block_rows": s.dens.neighbor_block_rows(s.n, s.D, 3)}


# ---- the other families, as functions of (dens, probe): run in-process and in the children of the forced forms -----------
def basic_programme(s, radii, fe=None, n_seg=3, rows=None):
    """populations (each radius alone, all together through Python and unsorted into the ABI, a row range, segment sums)
    and neighbours (all rows, the row range, segments merged both ways) of one case"""
    n = s.n
    lo, hi = rows if rows else (n // 3 + 5, max(n // 3 + 6, n - 41))
    lo, hi = min(lo, n - 1), min(max(hi, lo + 1), n)
    for r in radii:
        s.pops([r])
    s.pops(radii)
    s.pops(radii, abi=True)
    s.pops(radii, lo, hi)
    s.pop_segments(radii, n_seg)
    s.pop_segments(radii[:1], 2, abi=True)
    if fe is None:
        fe = fe_families.make("continuous", s.c, None, seed=n)
    s.nn(fe)
    s.nn(fe, lo, hi)
    s.nn_segments(fe, n_seg)


def gap_cases():
    """(what, coords, side, T, g) of the pruning-rule cases"""
    for D in (3, 10, 30):
        yield (f"gap plane D={D}",) + gap_sets(D, GAP_PLANE, "plane") + (GAP_PLANE,)
        yield (f"gap equal D={D}",) + gap_sets(D, GAP_PLANE, "equal") + (GAP_PLANE,)
        if D >= 5:
            yield (f"gap beyond D={D}",) + gap_sets(D, GAP_BEYOND, "beyond") + (GAP_BEYOND,)


def run_gaps(dens, probe, log=None):
    for what, c, side, T, g in gap_cases():
        s = Self(dens, probe, c, what=what)
        check_gap_case(s.d2, side, T)
        radii = gap_radii(T, g)
        want = expect_self_pops(s.d2x, radii)
        cross_at = (s.d2[np.ix_(~side, side)] == F32(T)).sum(axis=1)
        assert (want[1][~side] - want[0][~side] >= cross_at).all() and cross_at.any()   # (the float above T takes them in)
        s.pops(radii)
        info = dens.components_info(s.t)     # (of THIS population sweep: the neighbour sweeps partition again)
        basic_programme(s, radii)
        if "equal" in what:
            assert info["n_components"] == 1, (what, info)
        if log:
            log(what, info)


def run_tiny(dens, probe, widths=(3, 24), log=None):
    up = radius_for(np.nextafter(F32(2.0), F32(np.inf)))
    for D in widths:
        for n in tiny_sizes():
            s = Self(dens, probe, lattice(n, D, 300 + n), what=f"tiny n={n} D={D}")
            basic_programme(s, [1.0, up, 0.0, INF], n_seg=2, rows=(0, 1) if n < 3 else (n - 2, n))
            fe = fe_families.make("constant", s.c, None, seed=1)
            s.nn(fe)
            if log:
                log(s.what, s.tiles)


CUT_R = 3.0    # the largest radius of the component-cut cases; boxes 1, CUT_R - 1, CUT_R and CUT_R + 1 apart


def cut_components(k, sep):
    """components of a cut case: frames are joined over r_conn = r_max / 2 = 1.5 lattice steps in columns 0/1
    (dc_mfma.hip launch of components_kernel: `r_conn = sink_in ? r_max : 0.5f * r_max`), so clusters whose boxes are one
    step apart are ONE component and clusters 2 or more apart are k"""
    return 1 if sep <= 0.5 * CUT_R or components_off() else k


def components_off():
    """the process runs with DC_POP_COMPONENTS=0 (read once by the library): one component whatever the data"""
    import os
    return os.environ.get("DC_POP_COMPONENTS", "1")[:1] == "0"


def cut_cases():
    """(what, coords, k, sep) of the component-cut cases"""
    for D, k, sep in ((3, 2, 1.0), (10, 3, 1.0), (3, 2, CUT_R - 1), (3, 2, CUT_R), (3, 2, CUT_R + 1), (10, 2, CUT_R - 1), (10, 2, CUT_R),
                      (10, 2, CUT_R + 1), (24, 2, CUT_R), (10, 2, 40 * CUT_R), (3, 5, 40 * CUT_R)):
        yield f"cut D={D} k={k} sep={sep}", cluster_row(D, k, sep, seed=int(10 * D + sep)), k, sep


def cut_radii():
    """a multi-radius call whose LARGEST radius alone can join the sets: r2 = 1, 3 and 9"""
    return [1.0, radius_for(3.0), CUT_R]


def check_cut_case(c, d2x, k, sep):
    check_cluster_row(c, k, sep)
    which = np.floor((c[:, 0] + 1.0) / (5.0 + sep)).astype(int)
    cross = which[:, None] != which[None, :]
    with np.errstate(invalid="ignore"):
        inside = [int(((d2x < square(r)) & cross).sum()) for r in cut_radii()]
    want = [F32(sep * sep) < square(r) for r in cut_radii()]     # (the closest cross pairs are exactly sep apart)
    assert [n > 0 for n in inside] == want, ("broken component case", sep, inside)
    if sep == CUT_R:
        assert ((d2x == F32(CUT_R * CUT_R)) & cross).any(), "broken component case: no cross pair AT the largest radius"


def run_cuts(dens, probe, log=None):
    out = {}
    for what, c, k, sep in cut_cases():
        s = Self(dens, probe, c, what=what)
        check_cut_case(s.c, s.d2x, k, sep)
        radii = cut_radii()
        s.pops(radii)
        out[what] = dens.components_info(s.t)["n_components"]
        assert out[what] == cut_components(k, sep), (what, out[what])
        s.pops(radii[::-1], abi=True)
        s.pops([radii[2]])
        s.pops([radii[1]])
        for n_seg in (2, 3):
            s.pop_segments(radii, n_seg)
            s.pop_segments([radii[2]], n_seg)
        fe = fe_families.make("pops", s.c, expect_self_pops(s.d2x, [radii[2]])[0].astype(np.uint64), seed=1)
        s.nn(fe)
        s.nn_segments(fe, 3)
        if log:
            log(what, out[what])
    return out


def slot_cases():
    """(what, coords, expected components): more clusters than the 64 component slots -> one component, one origin; 36
    clusters -> 36 components (as tests/test_gpu_components.py pins them for blob clusters)"""
    yield "slots 10 x 10", cluster_grid(4, 10, 120.0, seed=5), 1
    yield "slots 6 x 6", cluster_grid(4, 6, 120.0, seed=6, rows=60), 36


def run_slots(dens, probe, log=None):
    for what, c, want in slot_cases():
        s = Self(dens, probe, c, what=what)
        radii = [1.0, radius_for(3.0), radius_for(np.nextafter(F32(2.0), F32(np.inf)))]
        s.pops(radii)
        info = dens.components_info(s.t)
        if log:
            log(what, info)
        assert info["n_components"] == (1 if components_off() else want), (what, info)
        s.pop_segments(radii, 3)
        s.pops(radii, 100, len(c) - 77, abi=True)


def run_emptiness(dens, probe, widths=(3, 10, 30)):
    for D in widths:
        c, fe, far, low = emptiness(D, 40 + D)
        s = Self(dens, probe, c, what=f"emptiness D={D}")
        exp = expect_self_nn(s.d2x, fe)
        assert exp[2][far] == low and exp[3][far] > 1.0e5, "broken case: the far frame's lower neighbour is not at the other end"
        assert (exp[1] >= 1.0e4).sum() >= 7, "broken case: no isolated frames"
        for f in (fe, fe_families.make("continuous", c, None, seed=D)):
            s.nn(f)
            s.nn(f, 11, s.n - 13)
            for n_seg in (2, 5):
                s.nn_segments(f, n_seg)
        s.pops([1.0, radius_for(3.0)])


def inplace_cases(D=24, n=2500):
    """-> (coords, [(name, in_place, far radius or None)]): tie radii AMONG the radii on each side of "a step does not fit fp16" -- the steps
    between the lowest lattice levels are a few scaled units; a radius of 400 lattice steps, far beyond the other radii and
    the data's extent, sets the scale by itself, and its step of nearly S r2max (6.5e4 .. 1e5 scaled units,
    dc_mfma_msym.hpp) passes the 60000 a step's fp16 pieces hold"""
    c = lattice(n, D, 100 + D)
    return c, [("steps fit", True, None), ("a step does not fit fp16", False, 400.0)]


def run_inplace(dens, probe, log=None):
    seen = set()
    for D in (24, 17):
        c, sides = inplace_cases(D)
        s = Self(dens, probe, c, what=f"in place D={D}")
        at, above, below = check_tie_case(s.d2x, D)
        for name, in_place, far in sides:
            radii = [above[0], at[0], above[1], at[1]] + ([far] if far else [])
            if far:
                radii = [radii[0], far] + radii[1:-1]       # (the far one among the others)
            for abi in (False, True):
                s.pops(radii, abi=abi)
                tiles, issued = s.tiles["pop"], dens.issued_mfmas(s.t.device)[0]
                if log:
                    log(s.what, name, abi, tiles, issued, nm_for(D))
                assert (issued > tiles * nm_for(D)) == in_place, (s.what, name, abi, tiles * nm_for(D), issued)
                seen.add(issued > tiles * nm_for(D))
            s.pop_segments(radii, 3)
            s.pops(radii, 37, s.n - 45)
    assert seen == {True, False}


# ---- unsorted radii against the leading-radius skip of the symmetric multi-radius sweep -------------------------------------
# dc_mfma_msym.hpp:165-175: with ASCENDING radii a chain (32 x 32 pairs) whose smallest accumulator lies above the
# threshold of radius kMsSkip - 1 (the second of eight) holds nothing of the leading two radii, and their strings are not
# formed; "radii in any other order: nothing is skipped".  A sweep that skipped on unsorted radii would lose the pairs of a
# LARGER leading radius in every chain that holds nothing of a smaller second one.  The dense lattices never show it: every
# tile pair near enough to matter holds exact duplicates (d2 = 0), so no chain is above any threshold.  This data has NO
# duplicates and many pairs at d2 = 1, 2, 3; the call leads with a radius above 3 and a radius of 0.5.
def sparse_lattice(D, n, seed):
    """distinct integer rows: base points of {0..3}^D, each with variants one step away in one or two columns; exact
    duplicates removed -> every d2 >= 1, small d2 well populated"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, (max(1, n // 6), D))
    rows = base[rng.integers(0, len(base), 2 * n)].copy()
    for k in range(2):
        col = rng.integers(0, D, len(rows))
        rows[np.arange(len(rows)), col] += rng.choice([-1, 0, 1], len(rows))
    rows = np.unique(rows, axis=0)
    rows = rows[rng.permutation(len(rows))[:n]]
    return np.ascontiguousarray(rows, dtype=np.float32)


def skip_radii(d2x):
    """eight unsorted radii: the float above 3 first, 0.5 second (below every pair), tie radii among the rest"""
    up3, up2 = radius_for(np.nextafter(F32(3.0), F32(np.inf))), radius_for(np.nextafter(F32(2.0), F32(np.inf)))
    for t in (1.0, 2.0, 3.0):
        assert (d2x == F32(t)).any(), f"broken skip case: no pair at d2 = {t}"
    return [up3, 0.5, 1.0, up2, radius_for(3.0), 0.75, 2.0, 1.25]


def check_skip_case(c, d2x):
    """conditions of a skip case on the referee's matrix: no pair below the SECOND radius; and, with the rows ordered on
    columns 0/1 as the sweep's cells are, at least a tenth of the off-diagonal 32 x 32 blocks that hold a pair inside the
    FIRST radius at all hold none inside the second -- chains a wrong skip would empty -- and they hold at least a tenth of
    all pairs inside the first radius"""
    radii = skip_radii(d2x)
    r0, r1 = square(radii[0]), square(radii[1])
    assert r0 > r1 and not (d2x < r1).any(), "broken skip case: pairs below the second radius"
    order = np.lexsort((c[:, 1], c[:, 0]))
    m = d2x[np.ix_(order, order)]
    n = len(c) // 32 * 32
    blocks = m[:n, :n].reshape(n // 32, 32, n // 32, 32).transpose(0, 2, 1, 3).reshape(n // 32, n // 32, -1)
    with np.errstate(invalid="ignore"):
        inside = (blocks < r0).sum(axis=2)
    off = ~np.eye(n // 32, dtype=bool)
    share = float((inside[off] > 0).mean())
    assert share >= 0.10 and inside[off].sum() >= 0.10 * inside.sum() > 0, ("broken skip case", share)
    return radii


def skip_cases():
    for D in (17, 24):
        yield f"skip D={D}", sparse_lattice(D, 2000, 900 + D)


def run_skip(dens, probe, log=None):
    """under DC_POP_SHARED=1 (kPopMsym at 4 and 5 MFMAs per chain): the unsorted call straight into the ABI for all rows
    and for three segments, a row range (kPopMulti), through Python (sorted on the way), and the same with a radius of 40
    in seventh place (all tile pairs kept: most chains hold nothing of ANY radius and are skipped rightly)"""
    for what, c in skip_cases():
        s = Self(dens, probe, c, what=what)
        radii = check_skip_case(s.c, s.d2x)
        for rad in (radii, radii[:6] + [40.0] + radii[7:]):
            s.pops(rad, abi=True)
            s.pop_segments(rad, 3, abi=True)
            s.pops(rad, 37, s.n - 45, abi=True)
            s.pops(rad)
        if log:
            log(what, s.tiles, dens.issued_mfmas(s.t.device))


def degenerate_cases(n=5000, d=10):
    """the cases of test_gpu_parity.test_degenerate_inputs_pruned_equals_direct, which takes them from here: ONE list for
    the comparison with the direct kernels there and the comparison with the probe in test_gpu_pruned_edges (the
    probe's n x n matrix is the referee of this whole module; 5000 rows are still cheap for it)"""
    rng = np.random.default_rng(5)
    two = np.concatenate([np.zeros((n // 2, d)), np.ones((n - n // 2, d)) * 1e3])
    lat = np.stack(np.meshgrid(np.arange(20), np.arange(20), np.arange(10)), -1).reshape(-1, 3) * 0.25
    return [
        ("identical rows", np.full((n, d), 0.37), [0.0, 1e-3, 1.0]),
        ("all zero", np.zeros((n, d)), [0.5]),
        ("two far points, tiny radius", two, [1e-6, 10.0]),
        ("radius beyond everything", two, [1e9]),
        ("1e15", rng.normal(size=(n, d)) * 1e15, [2e15, 5e15]),
        ("1e-15", rng.normal(size=(n, d)) * 1e-15, [2e-15, 5e-15]),
        ("constant and huge column", np.concatenate([rng.normal(size=(n, d - 2)), np.full((n, 1), 7.0),
                                                     rng.normal(size=(n, 1)) * 1e6], 1), [3.0, 1e6]),
        ("radius 1e-30", rng.normal(size=(n, d)), [1e-30, 3.0]),
        ("radius inf", rng.normal(size=(300, 3)), [float("inf")]),
        ("radius NaN", rng.normal(size=(n, d)), [float("nan")]),
        ("radius 1e20", rng.normal(size=(700, 5)), [1e20]),
        ("NaN and 1e20 among others", rng.normal(size=(n, d)), [3.0, float("nan"), 1e20, 0.5]),
        ("n = 1", rng.normal(size=(1, 7)), [1.0]),
        ("n = 2 identical", np.ones((2, 40)), [0.0, 1.0]),
        ("64 columns", rng.normal(size=(3000, 64)), [8.0, 11.0, 12.5]),
        ("lattice", lat, [0.25, 0.5, 0.3535534]),
    ]


def check_all_case_conditions(probe):
    """every generator's conditions on the referee's data, without a GPU -> number of cases checked"""
    count = 0
    for reduced in (False, True):
        for D, kind, n, transform in tie_plan(reduced):
            c, scale = tie_data(D, kind, n, 100 + D, transform)
            assert not self_flagged(c)
            at, above, below = check_tie_case(off_diagonal(probe.pairwise_d2(c)), D)
            radius_lists(at, above or at[1:], below, scale)
            count += 1
    for what, c, side, T, g in gap_cases():
        assert not self_flagged(c)
        check_gap_case(probe.pairwise_d2(c), side, T)
        gap_radii(T, g)
        count += 1
    for what, c, k, sep in cut_cases():
        assert not self_flagged(c)
        check_cut_case(c, off_diagonal(probe.pairwise_d2(c)), k, sep)
        count += 1
    for what, c, want in slot_cases():
        assert not self_flagged(c) and len(c) <= 4000
        count += 1
    for D in (3, 10, 30):
        c, fe, far, low = emptiness(D, 40 + D)
        exp = expect_self_nn(off_diagonal(probe.pairwise_d2(c)), fe)
        assert exp[2][far] == low and exp[3][far] > 1.0e5 and (exp[1] >= 1.0e4).sum() >= 7
        count += 1
    for what, c in skip_cases():
        assert not self_flagged(c) and len(c) >= 1500, (what, len(c))
        check_skip_case(c, off_diagonal(probe.pairwise_d2(c)))
        count += 1
    for D in (24, 17):
        c, sides = inplace_cases(D)
        at, above, below = check_tie_case(off_diagonal(probe.pairwise_d2(c)), D)
        assert len(above) >= 2 and len(at) >= 2
        count += 1
    flagged = {name for name, c, radii in degenerate_cases() if self_flagged(np.asarray(c, dtype=np.float32))}
    assert flagged == set(), flagged     # (1e15 stays below the 5e16 of the statistics pass: the matrix cores serve it)
    return count
