"""Ticketed placement of the per-wave pruned sweeps (DC_SWEEP_DISPATCH, clustering_amd/csrc/dc_mfma_kernels.hpp
for_each_unit): persistent workgroups draw their units -- a block of query groups x a reference share -- from
eight queues, their own first, then the others'.

Which workgroup runs a unit changes nothing of what the unit computes.  GPU (-m gpu): every case runs under
DC_SWEEP_DISPATCH=tickets and =static, each in a fresh child process (the switches are read once per process), and is held
three ways: tickets against static bit for bit, tickets against the CPU oracle, and the population sweep's tile-pair
counter (density.evaluated_tiles) equal in both modes.  The neighbour sweep's counter depends on when the shares of a
group publish their incumbents to each other and is not compared; its four arrays are.

The compared outputs: populations, nn_idx, hd_idx and the bits of nn_d2 and hd_d2.  The cases:
  blobs        4 993 x 10 in three blobs, all rows: fewer units than resident workgroups, groups no multiple of 8;
               segment 1 of 3 (and the three segments merged, for the oracle) and the row range [2000, 2300)
  blobs, many shares (DC_SHARE_FLOOR=16, DC_WAVE_TARGET=4000) on few workgroups: DC_SWEEP_SLOTS=8 -- every workgroup
               loops many times -- and DC_SWEEP_SLOTS=1 -- one workgroup drains all eight queues by stealing
  rows20k      20 000 x 10 with the same two overrides and no cap: more units than resident workgroups (and once more with
               DC_NN_COOP=0, which keeps the neighbour sweep's 39 shares per group out of the cooperative kernel)
  cols3 / cols12   3 000 x 3 (one MFMA per chain) and 3 000 x 12 (three: four waves per workgroup, the unit goes through
               LDS and the barriers)
  pairs        the radius graph's pair list (kSinkPairs) at 3 000 x 10, compared as a set
  nan          a row with a NaN: the header flag sends the call to the direct kernels, the persistent kernel leaves at
               once; the call after it (cols3 again) must still be right

CPU: tests/test_sweep_units.py holds the queues to the static grid."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("nn_idx", "nn_d2", "hd_idx", "hd_d2")
RADIUS = 0.2
RANGE = (2000, 2300)
SHARES = {"DC_SHARE_FLOOR": "16", "DC_WAVE_TARGET": "4000"}


# ---- the data ----------------------------------------------------------------------------------------------------------
def three_blobs(sizes, D, seed):
    """blobs (sigma 0.06) three units apart: components with origins of their own, the first smaller than a query group"""
    rng = np.random.default_rng(seed)
    parts = []
    for k, m in enumerate(sizes):
        x = rng.normal(0.0, 0.06, (m, D))
        x[:, 0] += 3.0 * k
        x[:, 1] -= 1.0 * k
        parts.append(x)
    c = np.concatenate(parts)
    return np.ascontiguousarray(c[rng.permutation(c.shape[0])], dtype=np.float32)


def two_blobs(n, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.08, (n, D))
    x[:, 0] += rng.integers(0, 2, n)
    x[rng.integers(0, n, n // 16)] = x[rng.integers(0, n, n // 16)]   # (duplicates: ties at d2 = 0)
    return np.ascontiguousarray(x, dtype=np.float32)


def make_data(name):
    if name in ("blobs", "blobs_parts"):
        return three_blobs((150, 2400, 2443), 10, seed=11)
    if name == "rows20k":
        return three_blobs((150, 9000, 10850), 10, seed=12)
    if name in ("cols3", "after_nan"):
        return two_blobs(3000, 3, seed=13)
    if name == "cols12":
        return two_blobs(3000, 12, seed=14)
    if name == "pairs":
        return two_blobs(3000, 10, seed=15)
    assert name == "nan"
    c = three_blobs((150, 2400, 2443), 10, seed=16)
    c[1234, 4] = np.nan
    return c


# ---- one case on the device (in a child: under the child's switches) -----------------------------------------------------
def run_case(dens, name):
    import torch
    c = make_data(name)
    ct = torch.from_numpy(c).cuda()
    dev = ct.device
    out = {}

    def bits(t):
        return t.cpu().numpy().view(np.uint32)

    if name == "pairs":
        pairs, pops = dens.radius_pairs(ct, RADIUS * RADIUS)
        out["pairs"] = pairs.cpu().numpy()
        out["pops"] = bits(pops)
        return out
    pops = dens.calculate_populations_partial(ct, [RADIUS], variant="pruned")
    out["all.pop_tiles"] = np.array([dens.evaluated_tiles(dev)[0]], np.int64)
    out["all.pops"] = bits(pops)
    fe = dens.calculate_free_energies(pops[0].contiguous())
    out["fe"] = bits(fe)
    for nm, a in zip(NAMES, dens.nearest_neighbors_partial(ct, fe, variant="pruned")):
        out["all." + nm] = bits(a)
    if name != "blobs_parts":
        return out
    # segment 1 of 3 as it comes, and the three segments merged as a sharded run merges them
    total, words = None, None
    for g in range(3):
        p = dens.calculate_populations_segment(ct, [RADIUS], g, 3, variant="pruned")
        tiles = dens.evaluated_tiles(dev)[0]
        nn = dens.nearest_neighbors_segment(ct, fe, g, 3, variant="pruned")
        if g == 1:
            out["seg1.pop_tiles"] = np.array([tiles], np.int64)
            out["seg1.pops"] = bits(p)
            for nm, a in zip(NAMES, nn):
                out["seg1." + nm] = bits(a)
        w = dens.pack_neighbors(*nn)
        total = p.clone() if total is None else total + p
        words = w if words is None else torch.minimum(words, w)
    out["merged.pops"] = bits(total)
    for nm, a in zip(NAMES, dens.unpack_neighbors(words)):
        out["merged." + nm] = bits(a)
    lo, hi = RANGE
    p = dens.calculate_populations_partial(ct, [RADIUS], lo, hi, variant="pruned")
    out["range.pop_tiles"] = np.array([dens.evaluated_tiles(dev)[0]], np.int64)
    out["range.pops"] = bits(p)
    for nm, a in zip(NAMES, dens.nearest_neighbors_partial(ct, fe, lo, hi, variant="pruned")):
        out["range." + nm] = bits(a)
    return out


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_sweep_tickets as T
from clustering_amd import density as dens
out = {}
for name in json.loads(sys.argv[2]):
    for k, v in T.run_case(dens, name).items():
        out[name + "/" + k] = v
np.savez(sys.argv[3], **out)
print("ok")
"""


def child(path, names, env):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(list(names)), path], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and "ok" in r.stdout, (env, r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    return {name: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")} for name in names}


# (nan, then cols3 once more: the call after a flagged one)
DEFAULT_CASES = ("blobs", "blobs_parts", "cols3", "cols12", "pairs", "nan", "after_nan")


def both_modes(tmp_path_factory, tag, names, env):
    d = tmp_path_factory.mktemp(tag)
    return (child(str(d / "tickets.npz"), names, dict(env, DC_SWEEP_DISPATCH="tickets")),
            child(str(d / "static.npz"), names, dict(env, DC_SWEEP_DISPATCH="static")))


@pytest.fixture(scope="module")
def default_switches(tmp_path_factory):
    return both_modes(tmp_path_factory, "tickets_default", DEFAULT_CASES, {})


@pytest.fixture(scope="module")
def many_shares(tmp_path_factory):
    """blobs and rows20k with many shares: (tickets, static)"""
    return both_modes(tmp_path_factory, "tickets_shares", ("blobs", "rows20k"), SHARES)


@pytest.fixture(scope="module")
def many_shares_no_coop(tmp_path_factory):
    return both_modes(tmp_path_factory, "tickets_nocoop", ("rows20k",), dict(SHARES, DC_NN_COOP="0"))


_expected = {}


def expected(oracle, name):
    """the oracle's populations, free energies and neighbours of a data set, computed once"""
    if name not in _expected:
        c = make_data(name)
        pops = oracle.populations(c, [RADIUS])
        fe = oracle.free_energies(pops[0])
        _expected[name] = (c, pops, fe, oracle.nearest_neighbors(c, fe))
    return _expected[name]


def nn_words(exp):
    return (exp[0].astype(np.uint32), np.ascontiguousarray(exp[1], np.float32).view(np.uint32),
            exp[2].astype(np.uint32), np.ascontiguousarray(exp[3], np.float32).view(np.uint32))


def same(tickets, static, what):
    """every array of a case bit for bit in both modes; the population counters equal (and not vacuous)"""
    assert sorted(tickets) == sorted(static), what
    for k in tickets:
        assert tickets[k].shape == static[k].shape and (tickets[k] == static[k]).all(), (what, k, "tickets against static")
        if k.endswith(".pop_tiles") and not what.startswith("nan"):
            assert int(tickets[k][0]) > 0, (what, k)


def hold_all_rows(oracle, name, tickets, static, what=None):
    what = what or name
    same(tickets, static, what)
    _, pops, fe, nn = expected(oracle, name)
    assert (tickets["all.pops"][0].astype(np.uint64) == pops[0]).all(), (what, "populations against the oracle")
    assert (tickets["fe"] == fe.view(np.uint32)).all(), (what, "free energies against the oracle")
    for nm, w in zip(NAMES, nn_words(nn)):
        assert (tickets["all." + nm] == w).all(), (what, nm, "against the oracle")
    print("%s: %d population tile pairs in both modes" % (what, int(tickets["all.pop_tiles"][0])))


@gpu
def test_fewer_units_than_workgroups(oracle, default_switches):
    """4 993 x 10 under the default switches: the grid is the unit count rounded down to 8, the rest is stolen"""
    hold_all_rows(oracle, "blobs", default_switches[0]["blobs"], default_switches[1]["blobs"])


@gpu
def test_segment_and_row_range(oracle, default_switches):
    """segment 1 of 3 (populations_segment / nearest_neighbors_segment) and the row range [2000, 2300) (.._partial)"""
    t, s = default_switches[0]["blobs_parts"], default_switches[1]["blobs_parts"]
    same(t, s, "blobs_parts")
    c, pops, fe, nn = expected(oracle, "blobs")
    assert (t["merged.pops"][0].astype(np.uint64) == pops[0]).all(), "the three segments' partial counts add up to the oracle's"
    for nm, w in zip(NAMES, nn_words(nn)):
        assert (t["merged." + nm] == w).all(), (nm, "three segments merged against the oracle")
    # segment 1 answers for its own rows only: "none" elsewhere, the oracle's values where it answers
    none = t["seg1.nn_idx"] == np.uint32(c.shape[0] + 1)
    assert 0 < none.sum() < c.shape[0]
    assert (t["seg1.nn_idx"][~none] == nn[0].astype(np.uint32)[~none]).all()
    lo, hi = RANGE
    part = oracle.populations(c, [RADIUS], lo, hi)
    assert (t["range.pops"][0].astype(np.uint64) == part[0]).all(), "row range: populations against the oracle"
    for nm, w in zip(NAMES, nn_words(oracle.nearest_neighbors(c, fe, lo, hi))):
        assert (t["range." + nm] == w).all(), (nm, "row range against the oracle")


@gpu
@pytest.mark.parametrize("slots", [8, 1])
def test_many_shares_on_few_workgroups(oracle, many_shares, tmp_path, slots):
    """eight workgroups loop many times each; ONE workgroup drains its own queue and then the seven others"""
    got = child(str(tmp_path / "slots.npz"), ("blobs",), dict(SHARES, DC_SWEEP_DISPATCH="tickets", DC_SWEEP_SLOTS=str(slots)))
    hold_all_rows(oracle, "blobs", got["blobs"], many_shares[1]["blobs"], what="blobs, %d workgroup(s)" % slots)
    # (the shares are there: more tile pairs' worth of units than under the default switches is not asserted -- the counter
    #  counts chains, not units -- but the uncapped ticketed run must agree too)
    same(many_shares[0]["blobs"], many_shares[1]["blobs"], "blobs, many shares")


@gpu
def test_more_units_than_workgroups(oracle, many_shares, many_shares_no_coop):
    """20 000 x 10, 39 shares per group: about 4 000 units for the chip's 2 048 resident one-wave workgroups"""
    hold_all_rows(oracle, "rows20k", many_shares[0]["rows20k"], many_shares[1]["rows20k"])
    hold_all_rows(oracle, "rows20k", many_shares_no_coop[0]["rows20k"], many_shares_no_coop[1]["rows20k"],
                  what="rows20k, DC_NN_COOP=0")


@gpu
@pytest.mark.parametrize("name", ["cols3", "cols12"])
def test_one_and_four_waves_per_workgroup(oracle, default_switches, name):
    """3 columns: one MFMA per chain, one wave per workgroup (readfirstlane); 12 columns: three MFMAs, four waves per
    workgroup -- the unit is broadcast through LDS between barriers that every wave reaches in every trip"""
    hold_all_rows(oracle, name, default_switches[0][name], default_switches[1][name])


@gpu
def test_pair_list(oracle, default_switches):
    """kSinkPairs: the same set of pairs in both modes, every pair once, and as many partners per frame as the oracle counts"""
    t, s = default_switches[0]["pairs"], default_switches[1]["pairs"]
    assert (t["pops"] == s["pops"]).all()

    def as_set(p):
        p = np.sort(p.astype(np.int64), axis=1)
        keys = p[:, 0] * (1 << 32) + p[:, 1]
        assert len(np.unique(keys)) == len(keys), "a pair is listed twice"
        return np.sort(keys)

    kt, ks = as_set(t["pairs"]), as_set(s["pairs"])
    assert len(kt) > 0 and len(kt) == len(ks) and (kt == ks).all()
    c, pops, _, _ = expected(oracle, "pairs")
    degree = np.bincount(t["pairs"].astype(np.int64).ravel(), minlength=c.shape[0])
    assert (degree.astype(np.uint64) + 1 == pops[0]).all(), "partners per frame against the oracle's populations"
    assert (t["pops"].astype(np.uint64) == pops[0]).all()


@gpu
def test_flagged_call_and_the_call_after_it(oracle, default_switches):
    """a NaN row: the direct kernels answer, the persistent kernels leave at once without drawing; the next call's
    counters start clean"""
    hold_all_rows(oracle, "nan", default_switches[0]["nan"], default_switches[1]["nan"])
    assert int(default_switches[0]["nan"]["all.pop_tiles"][0]) == 0, "the matrix-core sweep stood down"
    hold_all_rows(oracle, "after_nan", default_switches[0]["after_nan"], default_switches[1]["after_nan"])
    same(default_switches[0]["after_nan"], default_switches[0]["cols3"], "cols3 after the flagged call against cols3 before it")
