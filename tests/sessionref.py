"""Cases, referees and the runner of the resident-session edge tests (tests/test_gpu_session_edges.py, its one child process
and the GPU-free condition test tests/test_session_edge_cases.py).

The referee of everything a session hands out is the probe's canonical d2 matrix of the case's coordinates
(oracle/fastmath_probe.cpp) with the self-sweep conventions of include/dc_density.h restated in numpy (tests/prunedref.py);
free energies are Oracle.free_energies of the expected populations, sigma2 is Oracle.sigma2 of the expected nn_d2 (a double
sum in frame order), pair lists are the brute-force pair set of the matrix and a forest is held to its contract
(graphref.check_forest) -- never to another forest, and nothing to the call-by-call GPU path.  The data are integer
lattices (tests/graphref.py): exact in every summation order, with duplicates, tied nearest candidates and pairs exactly at
a radius.  Flow mirrors the session's state -- which populations and free energies are resident -- so that the expectation
of a step follows from the steps before it and not from what the library says.

Importing this module needs neither a GPU nor torch; only Flow touches the device."""
import numpy as np

import fe_families
from crossref import F32, bits, square
from graphref import INF, NAN, check_forest, clustered_lattice, keys, lattice, pairs_of, rank_of
from prunedref import (expect_self_nn, expect_self_pops, nn_tie_share, off_diagonal, radius_for, self_flagged,
                       tie_radii_of)

MAX_ROWS = 3000
POISON = {"nan": np.nan, "inf": np.inf, "6e16": 6.0e16}     # (6e16: beyond the 5e16 of the statistics pass, dc_prep.hpp)
FAMILIES = ("ties_ulp", "signed_zero", "inf", "nan")         # set_free_energies in the sessions of several devices
HIP_ERROR_MARK = "a session call returned DC_ERR_HIP:"    # (what a child process that met one leaves on stderr)
OPENED = [0]                                                 # sessions opened through open_flow (reported by the GPU module)


# ---- data ---------------------------------------------------------------------------------------------------------------
def data(kind, n, D, seed, poison=None):
    """n rows of the lattice (kind "lattice") or of five lattice clusters 64 apart ("clustered"); poison: ONE cell
    replaced by NaN / inf / 6e16 -- the statistics pass of a self sweep then flags the data"""
    c = (lattice if kind == "lattice" else clustered_lattice)(n, D, seed).reshape(n, D).astype(np.float32)
    if poison is not None:
        assert n >= 1
        c[(n // 2 + 1) % n, min(4, D - 1)] = POISON[poison]
    assert n <= MAX_ROWS
    return np.ascontiguousarray(c)


def sigma_data(n=400, D=3, seed=9):
    """a lattice and three frames about 4000 steps away along different axes (their d2 to the lattice are integers below 2^24, exact in every order):
    their nn_d2 of about 1.6e7 each add up beyond 2^24, where a FLOAT sum no longer takes in the many nn_d2 of 1 and 2 --
    sigma2 accumulated in float differs from the reference's double sum (checked by float_sum_differs)"""
    c = lattice(n, D, seed)
    far = np.zeros((3, D), dtype=np.float32)
    far[0, 0], far[1, 1], far[2, 0] = 4000.0, 4001.0, -3990.0
    c[[5, n // 2, n - 7]] = far
    return np.ascontiguousarray(c, dtype=np.float32)


def float_sum_differs(nn_d2):
    """True where the sum of nn_d2 in frame order differs between float and double accumulation"""
    acc32, acc64 = F32(0.0), 0.0
    for v in np.asarray(nn_d2, dtype=np.float32):
        acc32 = F32(acc32 + v)
        acc64 += float(v)
    return float(acc32) != acc64


class Ref:
    """one coordinate set and what the probe says about it"""

    def __init__(self, probe, oracle, c):
        self.c = np.ascontiguousarray(c, dtype=np.float32)
        self.n, self.D = self.c.shape
        self.oracle = oracle
        self.d2 = probe.pairwise_d2(self.c) if self.n else np.zeros((0, 0), dtype=np.float32)
        self.d2x = off_diagonal(self.d2) if self.n else self.d2
        self.flagged = self_flagged(self.c)
        self.wide = self.D > 64          # no matrix-core sweep, no workspace: the counters stay 0

    def pops(self, radii):
        return expect_self_pops(self.d2x, list(radii))

    def fe(self, pops_row):
        return self.oracle.free_energies(np.asarray(pops_row).astype(np.uint64))

    def nn(self, fe):
        return expect_self_nn(self.d2x, np.asarray(fe, dtype=np.float32))

    def sigma2(self, nn_d2):
        """compute_sigma2: the oracle's double sum in frame order (0 / 0 for no rows)"""
        return self.oracle.sigma2(nn_d2) if self.n else float("nan")

    def pairs(self, r2):
        return pairs_of(self.d2, r2)


# ---- radii --------------------------------------------------------------------------------------------------------------
def small_radii():
    """radii for the shapes too small for tie_radii_of's conditions: squares 1 and 4 (lattice levels) and the floats
    above 2 and 3"""
    above = [radius_for(np.nextafter(F32(t), F32(np.inf))) for t in (2.0, 3.0)]
    return [1.0, 2.0], [r for r in above if r is not None], []


def radii_of(ref, ties=None):
    """the radius lists of a case -> dict: at / above / below (radii whose squares are a lattice level, the float above,
    the float below; for cases with 500 rows or more from the case's own d2 matrix, else small_radii), and the calls
      one      [the float above the lowest level]
      multi3   three tie radii, unsorted
      multi9   nine radii, unsorted: tie radii at / above / below, 0, NaN, inf, 1e20 and a repeat
      r2       squared radii for pair lists and forests: the lowest level itself (its pairs stay out) and the float above
    ties: (at, above, below) of the unpoisoned data for a flagged case (its own matrix holds NaN / inf)"""
    if ties is None:
        ties = tie_radii_of(ref.d2x) if ref.n >= 500 else small_radii()
    at, above, below = ties
    up = above or at[1:]
    lo = below or at
    out = {"at": at, "above": above, "below": below, "one": [up[0]], "multi3": [up[0], at[0], at[-1]],
           "multi9": [at[-1], 0.0, up[0], INF, lo[0], NAN, 1e20, at[0], up[0]],
           "r2": {"at": float(square(at[0])), "above": float(square(up[0]))}}
    assert len(out["multi9"]) == 9
    return out


def count_lists(R):
    """radius counts 1, 9, 2, 17, 1 for ONE session (d_pops grows, shrinks in use, grows again): unsorted, with 0, NaN,
    inf, 1e20, a repeat and radii at, inside and outside the tie level"""
    at, up, lo = R["at"], R["above"] or R["at"][1:], R["below"] or R["at"]
    seventeen = [up[-1], 1e-30, at[0], 40.0, NAN, at[-1], 1e20, up[0], at[0], lo[0], 0.0, INF, lo[-1], up[0], 0.5, at[-1], up[-1]]
    lists = [[up[0]], R["multi9"], [at[-1], lo[0]], seventeen, [at[0]]]
    assert [len(x) for x in lists] == [1, 9, 2, 17, 1]
    return lists


# ---- call orders ----------------------------------------------------------------------------------------------------------
# a step: ("pops", key of radii_of or "lump", fetch) | ("fe", index or "last", fetch) | ("setfe", family) | ("nn",)
#         | ("pairs", "at" / "above") | ("forest", "at" / "above" / "lump", rank kind or "fe")
# "lump": the lumping radius fl32(sqrt(4 sigma2)) of the last neighbour call (density_clustering.cpp:649-673), for a forest
# r2 = 4 sigma2.  Each order names the pair of consecutive steps it was written for ("start": the first call of a session).
ORDERS = {
    "whole flow twice": ([("pops", "multi3", True), ("fe", 1, True), ("nn",), ("forest", "above", "fe"), ("pops", "multi9", True),
                          ("fe", "last", True), ("nn",)], ("forest", "pops")),
    "handed-in free energies, no populations ever": ([("setfe", "ties_ulp"), ("nn",), ("setfe", "nan"), ("nn",),
                                                      ("setfe", "continuous"), ("nn",)], ("setfe", "nn")),
    "pairs between two population calls": ([("pops", "multi3", True), ("pairs", "above"), ("pops", "one", True), ("fe", 0, True),
                                            ("nn",)], ("pairs", "pops")),
    "free energies survive the forest": ([("pops", "multi3", True), ("fe", 2, True), ("forest", "at", "random"), ("nn",)],
                                         ("forest", "nn")),
    "free energies survive the pair list": ([("pops", "multi9", False), ("fe", 4, True), ("pairs", "at"), ("nn",)],
                                            ("pairs", "nn")),
    "neighbours twice in a row": ([("pops", "one", True), ("fe", 0, False), ("nn",), ("nn",)], ("nn", "nn")),
    "forest as the first call": ([("forest", "above", "bit-reversed"), ("pops", "multi3", True), ("fe", 0, True), ("nn",)],
                                 ("start", "forest")),
    "forest, pairs, populations": ([("forest", "at", "reversed"), ("pairs", "above"), ("pops", "multi9", False), ("fe", 8, True),
                                    ("nn",), ("pops", "one", True)], ("pairs", "pops")),
    "the lumping flow": ([("pops", "multi3", True), ("fe", 0, True), ("nn",), ("pops", "lump", True), ("fe", 0, True), ("nn",),
                          ("forest", "lump", "fe")], ("nn", "pops")),
}
# ... reduced, for the sessions of several devices and the one-rank RCCL child: every kind of step and every hand-over between
# two sweeps of different kinds (the families of FAMILIES follow it in those tests)
REDUCED = [("forest", "above", "random"), ("pops", "multi9", True), ("fe", 4, True), ("nn",), ("forest", "at", "fe"),
           ("pops", "one", False), ("fe", 0, True), ("nn",), ("nn",)]
REDUCED_PAIRS = (("start", "forest"), ("forest", "pops"), ("pops", "fe"), ("fe", "nn"), ("nn", "forest"), ("nn", "nn"))


def step_pairs(steps):
    kinds = ["start"] + [s[0] for s in steps]
    return set(zip(kinds[:-1], kinds[1:]))


# ---- the case lists -------------------------------------------------------------------------------------------------------
# (name, kind, n, D, seed): the one-device cases of the call orders, the refusals, the radius counts and the optional outputs
ONE_DEVICE = {10: ("lattice D=10", "lattice", 1500, 10, 110), 24: ("clustered D=24", "clustered", 2200, 24, 124)}
TINY_ROWS = (0, 1, 2, 31, 33, 37)
# several "devices" on one GPU: (n, D, G, neighbour merge, poison)
MULTI = [
    (0, 3, 2, "allgather", None), (0, 70, 3, "allreduce", None), (1, 24, 5, "allgather", None), (1, 3, 2, "allreduce", None),
    (2, 64, 3, "allgather", None), (2, 70, 5, "allreduce", None), (2, 3, 5, "allgather", None),
    (37, 3, 5, "allgather", None), (37, 24, 3, "allreduce", None), (37, 64, 2, "allgather", None), (37, 70, 5, "allreduce", None),
    (37, 24, 5, "allgather", "nan"),
    (513, 3, 3, "allgather", None), (513, 24, 5, "allreduce", None), (513, 64, 2, "allreduce", None), (513, 70, 3, "allgather", None),
    (513, 24, 3, "allgather", "nan"), (513, 64, 5, "allgather", None),
    (2000, 3, 2, "allreduce", None), (2000, 24, 3, "allgather", None), (2000, 24, 5, "allreduce", None),
    (2000, 64, 5, "allgather", None), (2000, 64, 3, "allreduce", None), (2000, 70, 2, "allgather", None),
    (2000, 70, 3, "allreduce", None), (2000, 10, 5, "allreduce", "inf"), (2000, 24, 2, "allgather", "6e16"),
    (2000, 70, 3, "allgather", "inf"), (2000, 3, 5, "allgather", "6e16"),
]


def multi_id(case):
    n, D, G, merge, poison = case
    return f"n{n}-D{D}-G{G}-{merge}" + (f"-{poison}" if poison else "")


def multi_kind(D):
    return "clustered" if D in (24, 70) else "lattice"


def multi_data(case):
    """-> (coords, coords without the poisoned cell)"""
    n, D, G, merge, poison = case
    return data(multi_kind(D), n, D, 500 + D + n, poison), data(multi_kind(D), n, D, 500 + D + n)


def check_all_case_conditions(probe, oracle):
    """every case's conditions on the referee's data, without a GPU -> number of cases checked"""
    count = 0
    rows = set()
    for D, (name, kind, n, d, seed) in ONE_DEVICE.items():
        ref = Ref(probe, oracle, data(kind, n, d, seed))
        assert not ref.flagged and d == D and 1500 <= n <= 2500
        R = radii_of(ref)     # (tie_radii_of: pairs AT every level used, pairs one float below the float above, pairs below)
        assert len(R["above"]) >= 2 and len(R["below"]) >= 1, (name, R)
        share = nn_tie_share(ref.d2x)
        assert share >= 0.10, f"{name}: only {share:.3f} of the queries have tied nearest candidates at d2 > 0"
        for r2 in R["r2"].values():
            assert 0 < len(ref.pairs(r2)) < 400000, (name, r2, len(ref.pairs(r2)))
        with np.errstate(invalid="ignore"):
            assert (ref.d2x == F32(R["r2"]["at"])).any() and (ref.d2x < F32(R["r2"]["at"])).any()
        for lst in count_lists(R):
            assert all(r is not None for r in lst)
        want = ref.pops(R["multi3"])
        assert (want[1] < want[0]).any(), name     # (the level's own pairs are inside the float above it only)
        rows.add(n)
        count += 1
    for n in TINY_ROWS:
        for D in (3, 24):
            ref = Ref(probe, oracle, data("lattice", n, D, 300 + n))
            assert not ref.flagged
            radii_of(ref)
            rows.add(n)
            count += 1
    ref = Ref(probe, oracle, sigma_data())
    assert not ref.flagged
    nn_d2 = ref.nn(np.zeros(ref.n, dtype=np.float32))[1]
    assert nn_d2.max() < 2.0 ** 24     # (every d2 that can be a result is an exact integer)
    assert float_sum_differs(nn_d2) and (nn_d2 >= 1.5e7).sum() == 3, "broken sigma2 case: a float sum would do"
    count += 1
    seen = {"G": set(), "D": set(), "merge": set(), "poison": set()}
    for case in MULTI:
        n, D, G, merge, poison = case
        c, clean = multi_data(case)
        assert self_flagged(c) == (poison is not None) and not self_flagged(clean), multi_id(case)
        assert G <= 5 and n <= MAX_ROWS
        ref = Ref(probe, oracle, clean)
        R = radii_of(ref)
        if n >= 500 and D >= 10:
            assert nn_tie_share(ref.d2x) >= 0.10, multi_id(case)
        if n >= 500:
            assert 0 < len(ref.pairs(R["r2"]["above"])) < 400000, multi_id(case)
        if n >= 37:     # tied free energies among the candidates: the families with ties hand in repeated values
            for name in ("ties_ulp", "signed_zero"):
                fe = fe_families.make(name, c, None, seed=D)
                assert len(np.unique(fe)) < len(fe), (multi_id(case), name)
        for key, v in zip(("G", "D", "merge", "poison"), (G, D, merge, poison)):
            seen[key].add(v)
        rows.add(n)
        count += 1
    assert seen["G"] == {2, 3, 5} and seen["D"] >= {3, 24, 64, 70} and seen["merge"] == {"allgather", "allreduce"}
    assert seen["poison"] == {None, "nan", "inf", "6e16"}
    # more segments than query groups (a group holds at most 512 rows, prunedref.Self.owns_a_group): devices without a group
    assert any(G > -(-n // 512) for n, D, G, m, p in MULTI if n > 0)
    assert rows >= {0, 1, 2, 31, 33, 37, 513} and any(1500 <= n <= 2500 for n in rows) and max(rows) <= MAX_ROWS
    for name, (steps, pair) in ORDERS.items():
        assert pair in step_pairs(steps), (name, pair)
        count += 1
    assert set(REDUCED_PAIRS) <= step_pairs(REDUCED)
    return count


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def same_ints(got, want, what):
    g, w = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not (g == w).all():
        bad = np.argwhere(g != w)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} entries differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}")


def same_floats(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not (g == w).all():
        bad = np.flatnonzero(g != w)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} floats differ by bits, first at row {bad[0]}: "
                             f"{np.asarray(got)[bad[0]]!r} != {np.asarray(want)[bad[0]]!r}")


def same_double(got, want, what):
    a, b = np.float64(got), np.float64(want)
    assert (np.isnan(a) and np.isnan(b)) or a.view(np.uint64) == b.view(np.uint64), (what, got, want)


def rank_from_fe(fe):
    """the rank a host derives from free energies (ties by frame id)"""
    return np.argsort(np.argsort(fe, kind="stable"), kind="stable").astype(np.uint32)


# ---- the runner -----------------------------------------------------------------------------------------------------------
class Flow:
    """a session and the model of its state: `res` the expected resident populations (None: none -- never computed, or
    overwritten by a pair list or a forest), `fe_now` the expected resident free energies (None: none, or dropped by a
    population call).  Every method calls the session, holds what comes back to the referee over ALL rows and -- for the
    sweeps -- checks who answered."""

    def __init__(self, dens, ref, session, what, R=None):
        self.dens, self.ref, self.s, self.what = dens, ref, session, what
        self.R = R
        self.res = None
        self.fe_now = None
        self.sigma2 = None
        assert session.n_rows == ref.n and session.n_cols == ref.D

    # -- plumbing
    def call(self, fn, *a, **kw):
        """a session call; DC_ERR_HIP ends the whole run: nothing more is started on a device after a HIP error"""
        from clustering_amd import capi
        try:
            return fn(*a, **kw)
        except capi.DensityLibraryError as e:
            if e.status == capi.DC_ERR_HIP:
                import pytest
                pytest.exit(f"{HIP_ERROR_MARK} {self.what}: {e}", returncode=3)
            raise

    def refused(self, fn, *a, **kw):
        """the call must come back with DC_ERR_INVALID_ARGUMENT and a message; the model stays as it is"""
        from clustering_amd import capi
        try:
            self.call(fn, *a, **kw)
        except capi.DensityLibraryError as e:
            assert e.status == capi.DC_ERR_INVALID_ARGUMENT, (self.what, e.status, e.detail)
            assert e.detail.strip(), (self.what, "refused without a message")
            return e.detail
        raise AssertionError((self.what, "the call was not refused", getattr(fn, "__name__", fn), a))

    def who(self, kind, step, radii=None, fe=None):
        """the rule of prunedref.Self.answered on dc_hip_session_counters (the sum over the session's devices): unflagged
        data of at most 64 columns is answered by the pruned matrix-core sweep -- evaluated tiles > 0 after populations
        with some radius that squares to more than 0, and after neighbours of 2 rows or more without a NaN free energy;
        flagged data, wide rows and NaN free energies: 0 tiles"""
        if self.ref.n == 0:
            return
        tiles = self.call(self.s.counters)[0 if kind == "pop" else 1]
        fe_nan = fe is not None and bool(np.isnan(fe).any())
        if self.ref.flagged or self.ref.wide or fe_nan:
            assert tiles == 0, (self.what, step, "the exact kernel should have answered", tiles)
        elif kind == "pop":
            with np.errstate(invalid="ignore"):
                some = bool((np.array([square(r) for r in radii]) > 0).any())
            assert (tiles > 0) == some, (self.what, step, "evaluated tiles", tiles, "radii", radii)
        elif self.ref.n >= 2:
            assert tiles > 0, (self.what, step, "the session is on the exact kernels: evaluated tiles", tiles)

    # -- the steps
    def pops(self, radii, fetch=True, step="populations"):
        radii = [float(r) for r in radii]
        got = self.call(self.s.populations, radii, fetch=fetch)
        self.res, self.fe_now = self.ref.pops(radii), None
        if fetch:
            same_ints(got, self.res, (self.what, step, radii))
        self.who("pop", step, radii=radii)
        return self.res

    def fe(self, k, fetch=True, step="free energies"):
        assert self.res is not None, "the model holds no resident populations"
        k = len(self.res) - 1 if k == "last" else k
        want = self.ref.fe(self.res[k])
        got, mx = self.call(self.s.free_energies, k, fetch=fetch, max_pop=True)
        if self.ref.n:
            assert mx == int(self.res[k].max()), (self.what, step, "max_pop", mx, int(self.res[k].max()))
        if fetch:
            same_floats(got, want, (self.what, step, k))
        self.fe_now = want
        return want

    def set_fe(self, name, seed=0):
        pops = self.res[0].astype(np.uint64) if self.res is not None else None
        fe = fe_families.make(name, self.ref.c, pops, seed=seed)
        self.call(self.s.set_free_energies, fe)
        self.fe_now = fe
        return fe

    def nn(self, step="neighbours", **outputs):
        """outputs: nn_idx= / nn_d2= / hd_idx= / hd_d2= / sigma2= False for a NULL pointer"""
        assert self.fe_now is not None or self.ref.n == 0, "the model holds no resident free energies"
        got = self.call(self.s.nearest_neighbors, **outputs)
        want = self.ref.nn(self.fe_now if self.ref.n else np.zeros(0, dtype=np.float32))
        s2 = self.ref.sigma2(want[1])
        for k, name in enumerate(("nn_idx", "nn_d2", "hd_idx", "hd_d2")):
            if not outputs.get(name, True):
                assert got[k] is None
            elif k % 2 == 0:
                same_ints(got[k], want[k], (self.what, step, name))
            else:
                same_floats(got[k], want[k], (self.what, step, name))
        if outputs.get("sigma2", True):
            same_double(got[4], s2, (self.what, step, "sigma2"))
        self.sigma2 = s2
        self.who("nn", step, fe=self.fe_now)
        return want, s2

    def pairs(self, r2, step="pair list"):
        """the count alone (no buffer), a buffer of exactly the count, and one that is too small: the count is that of all
        pairs, what is written are distinct pairs of the graph"""
        want = self.ref.pairs(r2)
        n = max(self.ref.n, 1)
        self.res = None
        count, none = self.call(self.s.radius_pairs, r2, 0)
        assert count == len(want) and len(none) == 0, (self.what, step, r2, "count", count, len(want))
        count, got = self.call(self.s.radius_pairs, r2, len(want))
        assert count == len(want), (self.what, step, r2, "count", count, len(want))
        same_ints(np.sort(keys(got, n)), keys(want, n), (self.what, step, r2, "pairs"))
        if len(want) >= 2:
            count, part = self.call(self.s.radius_pairs, r2, len(want) // 2)
            pk = keys(part, n)
            assert count == len(want) and len(part) == len(want) // 2 and len(np.unique(pk)) == len(pk), (self.what, step, r2)
            assert np.isin(pk, keys(want, n)).all(), (self.what, step, r2, "a pair that is not in the graph")
        return want

    def forest(self, r2, rank, step="forest"):
        edges, rounds = self.call(self.s.radius_forest, r2, rank)
        self.res = None
        if self.ref.n <= 1:
            assert len(edges) == 0 and rounds == 0, (self.what, step)
            return edges
        check_forest(self.ref.n, self.ref.pairs(r2), rank, edges, rounds)
        return edges

    # -- programmes
    def run(self, steps):
        R = self.R
        for k, st in enumerate(steps):
            step = f"step {k} {st}"
            with np.errstate(over="ignore", invalid="ignore"):     # (one row: sigma2 = FLT_MAX; no rows: NaN)
                lump_r, lump_r2 = (float(F32(np.sqrt(4.0 * self.sigma2))), float(F32(4.0 * self.sigma2))) if self.sigma2 is not None else (None, None)
            if st[0] == "pops":
                radii = [lump_r] if st[1] == "lump" else R[st[1]]
                self.pops(radii, fetch=st[2], step=step)
            elif st[0] == "fe":
                self.fe(st[1], fetch=st[2], step=step)
            elif st[0] == "setfe":
                self.set_fe(st[1], seed=k)
            elif st[0] == "nn":
                self.nn(step=step)
            elif st[0] == "pairs":
                self.pairs(R["r2"][st[1]], step=step)
            elif st[0] == "forest":
                r2 = lump_r2 if st[1] == "lump" else R["r2"][st[1]]
                rank = rank_from_fe(self.fe_now) if st[2] == "fe" else rank_of(st[2], self.ref.n, seed=k)
                self.forest(r2, rank, step=step)
            else:
                raise AssertionError(st)

    def reduced(self, families=FAMILIES):
        """the reduced programme of a session of several devices (and of the one-rank RCCL child): REDUCED, the free-energy
        families with ties, signed zeros, inf and NaN handed in, and a pair list -- which overwrites the populations of
        device 0 alone -- followed by populations, free energies and neighbours"""
        self.run(REDUCED)
        for k, name in enumerate(families):
            self.set_fe(name, seed=self.ref.D + k)
            self.nn(step=f"neighbours under {name}")
        self.pairs(self.R["r2"]["above"])
        self.pops(self.R["multi3"], step="populations after the pair list")
        self.fe(2)
        self.nn(step="neighbours after the pair list")


def open_flow(dens, ref, what, R=None, **session_args):
    """-> Flow over a new session (a context manager through .s)"""
    OPENED[0] += 1
    return Flow(dens, ref, dens.Session(ref.c, **session_args), what, R=R)
