"""GPU (-m gpu): the PRUNED matrix-core self sweeps -- what DC_VARIANT_AUTO answers with -- in every form at ties and
pruning edges, against the probe's canonical d2 matrix (tests/prunedref.py: the self-sweep conventions of
include/dc_density.h restated in numpy) and never against another GPU variant.

  ties      integer lattices whose d2 are exact in every summation order (tests/graphref.py), plain and scaled by 2^-40 /
            2^20 / shifted by 1024, at 1 .. 64 columns (1 .. 13 MFMAs per chain); radii whose squares are a lattice
            level (its pairs stay outside: the strict <), the float above it (pairs one float inside) and the float below,
            alone and in unsorted calls of 3, 8 and 11 radii with 0, 1e-30, inf, 1e20, NaN and a repeated radius, through
            Python and straight into the C ABI; all rows, row ranges inside a tile and a query group, sums over 2, 3, 5
            and more segments than query groups; neighbours under free energies of several origins with at least 10 % of
            the queries tied at a positive minimal d2, for all rows, a row range and segments merged both ways
  forms     the same in child processes under the switch sets of test_gpu_parity.test_sweep_forms_agree
  pruning   two sets at a box gap of exactly g with the closest cross pairs AT the radius and one float inside it, the
            distance partly in other columns, sets equal in columns 0/1; the component cut at r_max - 1, r_max, r_max + 1
            and with more clusters than component slots; neighbours across emptiness; tiny shapes
  who       after every call: the statistics flag word is 0 and the sweep evaluated tiles, or -- where the case trips the
            flag -- the word is set and no tile was evaluated; the expected side comes from the data
            (prunedref.self_flagged restates stats_kernel of dc_prep.hpp)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import prunedref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dens():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from clustering_amd import density
    return density


@pytest.fixture(scope="module")
def probe():
    from clustering_amd import capi
    from oracle.oracle import Probe
    return Probe(capi.CANON_ORDER)


def log(*a):
    print("pruned-edges:", *a, flush=True)


# ---- the default form, in this process ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.tie_plan(), ids=lambda c: f"{c[1]}-D{c[0]}-{c[3][0].replace(' ', '')}")
def test_ties_at_the_radius(dens, probe, case):
    """every width, the lattice and the clustered lattice by turns, plain and under one other transform by turns: the
    whole programme of prunedref.Self.tie_programme"""
    P.run_ties(dens, probe, [case], log=log)


def test_box_gap_exactly_at_the_radius(dens, probe):
    """two sets whose boxes are exactly g apart with the closest cross pairs AT r2 = g^2 (outside) and inside the float
    above it; the same with part of the distance in columns 2 .. 4 (the plane test keeps the pair, the full d2 decides);
    sets equal in columns 0/1 (one component).  Who counts the cross pairs depends on the partition the sweep logs here:
    within one component the matrix-core tile rule (kept iff box_gap2 < r2max * 1.0001f), between two components the
    exact exchange behind the adjacency mask (pop_cross_kernel).  The child of DC_POP_COMPONENTS=0 (test_forms) runs the
    same cases as one component, i.e. through the tile rule for sure.
    What these cases can see of the rule: the boxes are integers, so box_gap2 is exact and a lower bound of every d2
    behind it -- no pair inside r2 has a tile pair with box_gap2 >= r2max, and dropping the 1.0001f margin alone is not
    observable with exact boxes (the margin pays for ROUNDED boxes and radii).  A rule that prunes too early is: far2 =
    r2max / 1.0001f loses the pairs at g^2 under r2 = the float above g^2, and these cases fail."""
    P.run_gaps(dens, probe, log=log)


def test_component_cut(dens, probe):
    """lattice clusters whose boxes are r_max - 1, r_max and r_max + 1 apart (cross pairs inside the LARGEST radius of a
    three-radius call only, exactly at it, none), and 40 r_max apart: populations of all rows, unsorted into the ABI,
    one radius, segment sums, neighbours.  Two edges are met: the component CUT (frames are joined over r_max / 2 = 1.5
    lattice steps in columns 0/1: clusters one step apart are one component, clusters 2 or more apart one each --
    prunedref.cut_components, asserted on components_info by run_cuts) and, at r_max - 1 / r_max / r_max + 1, the edge of
    the ADJACENCY mask between separate components (boxes closer than r_max exchange their cross pairs through the exact
    kernel; at r_max and beyond there are none), held to the referee through the populations."""
    got = P.run_cuts(dens, probe, log=log)
    assert set(got.values()) >= {1, 2, 5}, got


def test_more_clusters_than_component_slots(dens, probe):
    P.run_slots(dens, probe, log=log)


def test_neighbours_across_emptiness(dens, probe):
    """isolated frames whose nearest neighbour is 100 lattice steps away, and a frame whose only neighbour of lower free
    energy lies at the other end of the data: indices and d2 bits, all rows, a row range, 2 and 5 segments"""
    P.run_emptiness(dens, probe)


def test_tiny_shapes(dens, probe):
    """n = 1, 2, 31, 32, 33, 1025 and 3073 (one real row in the last tile and in the last query group)"""
    P.run_tiny(dens, probe, log=log)


def test_statistics_flag_hands_over_and_back(dens, probe):
    """one element beyond 5e16, one NaN, one inf: the flag is set, no tile is evaluated and the exact kernel gives the
    probe's values; the next call on clean data is answered by the matrix cores again.  5e16 itself is not beyond."""
    base = P.lattice(1500, 10, 77)
    for what, value in (("6e16", 6.0e16), ("NaN", np.nan), ("-inf", -np.inf)):
        c = base.copy()
        c[701, 4] = value
        s = P.Self(dens, probe, c, flagged=True, what=f"flagged by {what}")
        P.basic_programme(s, [1.0, P.radius_for(3.0), P.INF])
    c = base.copy()
    c[701, 4] = 5.0e16
    P.basic_programme(P.Self(dens, probe, c, what="5e16 is within the limit"), [1.0, 1.0e17])
    P.basic_programme(P.Self(dens, probe, base, what="clean after the flag"), [1.0, P.radius_for(3.0)])


# ---- the forced forms, one child process each (the switches are read once per process) ------------------------------------
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
from clustering_amd import capi, density as dens
from oracle.oracle import Probe
import prunedref as P
what = sys.argv[2]
assert capi.lib.dc_hip_canon_order().decode() == capi.CANON_ORDER
probe = Probe(capi.CANON_ORDER)
out = {}
if what == "forms":
    out = P.run_ties(dens, probe, P.tie_plan(reduced=True))
    P.run_tiny(dens, probe, widths=(24,))
    P.run_gaps(dens, probe)
    P.run_cuts(dens, probe)
    P.run_slots(dens, probe)
    P.run_emptiness(dens, probe)
elif what == "inplace":
    P.run_inplace(dens, probe, log=lambda *a: print("pruned-edges:", *a, file=sys.stderr))
elif what == "skip":
    P.run_skip(dens, probe, log=lambda *a: print("pruned-edges:", *a, file=sys.stderr))
elif what == "orders":
    out = P.run_ties(dens, probe, P.tie_plan(reduced=True)[1:4], families=("continuous",))
    # ... and blobs, whose d2 depend on the order: the probe of THIS order is the referee
    from clustering_amd.synth import gaussian_blobs
    from crossref import bits, radius
    differ = 0
    for D in (9, 24):
        c = gaussian_blobs(1800, D, seed=600 + D)
        c[:200] = c[900:1100]
        s = P.Self(dens, probe, c, what=f"blobs D={D} {capi.CANON_ORDER}")
        differ += int((bits(s.d2) != bits(Probe("sse2").pairwise_d2(c))).sum())
        P.basic_programme(s, [radius(D), 0.5 * radius(D), 2.0 * radius(D)])
    assert differ > 0, "the orders never differ on these blobs: the test would not tell them apart"
print("PRUNED " + json.dumps(out))
"""

FORMS = {
    "default": {},
    "one-sided": {"DC_POP_SYM": "0"},
    "one wave": {"DC_WAVES_PER_GROUP": "1"},
    "four waves": {"DC_WAVES_PER_GROUP": "4"},
    "pop shared": {"DC_POP_SHARED": "1"},
    "pop and nn shared": {"DC_POP_SHARED": "1", "DC_NN_SHARED": "1"},
    "coop floor 8": {"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "8"},
    "coop floor 16": {"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "16"},
    "coop floor 40": {"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "40"},
    "no coop floor 16": {"DC_NN_COOP": "0", "DC_SHARE_FLOOR": "16"},
    "no components": {"DC_POP_COMPONENTS": "0"},
}
_results = {}


def child(what, extra, timeout=900):
    env = dict(os.environ, **extra)
    if "DC_CANON_ORDER" in extra:
        env.pop("DC_LIB_PATH", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, what], capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):    # the child died on the GPU: nothing more is started on it
        pytest.exit(f"child {what} {extra} ended with status {r.returncode}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, (what, extra, r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("PRUNED ")]
    assert lines, (what, extra, r.stdout[-500:], r.stderr[-1500:])
    if r.stderr.strip():
        log(r.stderr.strip()[-1500:])
    return json.loads(lines[-1][7:])


def form(name):
    if name not in _results:
        _results[name] = child("forms", FORMS[name])
        log(name, json.dumps(_results[name]))
    return _results[name]


@pytest.mark.parametrize("name", list(FORMS))
def test_forms(name):
    """under one switch set: the reduced tie plan (3, 10, 17, 24, 40 and 64 columns: 1, 2, 4, 5, 8 and 13 MFMAs per
    chain -- the per-wave forms only, the multi-radius forms, the shared-operand forms with one radius and of the
    neighbour sweep, the per-wave forms again; one transform per width, all free-energy families), the tiny shapes at 24
    columns, the box-gap, component-cut, slot and emptiness cases.  Left out against the default form: the second
    transform of every width, widths 1 and 30, the tiny shapes at 3 columns, the statistics-flag and degenerate cases
    (no switch bears on who answers)"""
    form(name)


def test_the_switches_change_the_sweeps():
    """What the library's own counters can tell about the forms:
      DC_POP_SYM=0          the one-sided one-radius sweep evaluates more tiles than the symmetric one (every unordered
                            pair of groups once)
      DC_POP_SHARED=1       at 3 .. 8 MFMAs per chain a five-radius call is ONE multi-radius sweep with in-place
                            thresholds: it issues more MFMAs than tiles x MFMAs per chain, the default (one per-wave sweep
                            per radius) does not
      DC_POP_COMPONENTS=0   one component where the default finds several (the clustered lattices)
    No counter tells DC_WAVES_PER_GROUP, DC_NN_COOP / DC_SHARE_FLOOR or DC_NN_SHARED apart from the default (the
    evaluated tiles of the neighbour sweep depend on the shares' rings, not on who runs them): those forms are only held
    to the referee."""
    base, one_sided, shared, flat = form("default"), form("one-sided"), form("pop shared"), form("no components")
    for case, b in base.items():
        nm = b["nm"]
        assert b["one"][0] < one_sided[case]["one"][0], (case, b, one_sided[case])
        if 3 <= nm <= 8:
            assert shared[case]["five"][1] > shared[case]["five"][0] * nm, (case, shared[case])
            assert b["five"][1] <= b["five"][0] * nm, (case, b)
        if "clustered" in case:
            assert b["components"] > 1 and flat[case]["components"] == 1, (case, b, flat[case])


def test_multi_radius_in_place_edge():
    """tie radii among the radii of the symmetric multi-radius sweep on each side of "a step does not fit fp16"; the
    instance is read off the issued-MFMA count (dc_hip_workspace_mfma_counters_dev)"""
    child("inplace", {"DC_POP_SHARED": "1"})


def test_unsorted_radii_against_the_leading_radius_skip():
    """the symmetric multi-radius sweep "leaves out the leading radii a chain holds nothing of" for ascending radii only
    (dc_mfma_msym.hpp:165-175).  Data without duplicates (prunedref.sparse_lattice) and eight unsorted radii led by a
    large and a tiny one, straight into dc_hip_populations_dev / _segment_dev: a skip decided on unsorted radii would
    empty the first radius in most chains.  The dense lattices of the tie cases cannot show that (every near tile pair
    holds d2 = 0)."""
    child("skip", {"DC_POP_SHARED": "1"})


@pytest.mark.parametrize("order", ["avx", "fma"])
def test_pruned_sweeps_in_the_other_orders(order):
    """the avx / fma libraries (one process binds one library): two tie cases (lattice d2 are the same in every order) and
    blobs against the probe of that order"""
    if not os.path.exists(os.path.join(ROOT, "clustering_amd", "lib_" + order, "libdcdensity.so")):
        pytest.fail(f"clustering_amd/lib_{order}/libdcdensity.so is missing: __graft_entry__.build() makes it")
    child("orders", {"DC_CANON_ORDER": order})


# ---- the degenerate inputs of test_gpu_parity, with the probe as referee and the who-answered check ------------------------
@pytest.mark.parametrize("k", range(len(P.degenerate_cases())), ids=[c[0].replace(" ", "-") for c in P.degenerate_cases()])
def test_degenerate_inputs_against_the_probe(dens, probe, k):
    """the cases of test_degenerate_inputs_pruned_equals_direct (one list, prunedref.degenerate_cases) against the probe's
    n x n matrix -- the referee of this whole module, still cheap at 5000 rows -- instead of the direct kernels, each
    with the who-answered check: none of them trips the statistics flag of a pruned call (coordinates of 1e15 stay below
    its 5e16), so the matrix cores serve every one"""
    name, c, radii = P.degenerate_cases()[k]
    s = P.Self(dens, probe, c, flagged=False, what=name)
    s.pops(radii)
    s.pops(radii, abi=True)
    pops = P.expect_self_pops(s.d2x, radii[:1])[0].astype(np.uint64)
    import fe_families
    s.nn(fe_families.make("pops", s.c, pops))
    log(name, "tiles", s.tiles)
