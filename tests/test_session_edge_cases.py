"""Without a GPU: every case of tests/test_gpu_session_edges.py is built and its conditions are checked on the referee's
data (tests/sessionref.py) -- the tie radii have pairs at, one float inside and outside their level, at least 10 % of the
queries have tied nearest candidates at a positive d2, the handed-in free energies repeat values, the flagged cases trip the
statistics flag and the others do not, the row counts 0, 1, 2, 31, 33, 37, 513 and 1500 .. 2500 occur and none exceeds 3000,
some session has more devices than query groups, and every call order holds the pair of steps it was written for."""
import subprocess
import sys
import os

import numpy as np

import sessionref as S


def test_the_helper_needs_neither_torch_nor_a_gpu():
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import sessionref; "
            "assert 'torch' not in sys.modules, 'sessionref imports torch'") % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_case_conditions(probe, oracle):
    assert S.check_all_case_conditions(probe, oracle) >= 50


def test_every_order_names_a_step_pair_it_contains():
    for name, (steps, pair) in S.ORDERS.items():
        assert pair in S.step_pairs(steps), name
    assert ("start", "setfe") in S.step_pairs(S.ORDERS["handed-in free energies, no populations ever"][0])
    assert not any(s[0] == "pops" for s in S.ORDERS["handed-in free energies, no populations ever"][0])
    lump = S.ORDERS["the lumping flow"][0]
    assert ("pops", "lump", True) in lump and lump.index(("pops", "lump", True)) > lump.index(("nn",))


def test_the_model_follows_the_session_contract(probe, oracle):
    """the referee on five frames whose values are known by hand: populations count the frame itself, a pair AT the radius
    stays out, sigma2 is the mean of nn_d2, a pair list is strict"""
    c = np.array([[0, 0], [1, 0], [0, 1], [0, 0], [5, 5]], dtype=np.float32)
    ref = S.Ref(probe, oracle, c)
    assert ref.pops([1.0, 1.5])[0].tolist() == [2, 1, 1, 2, 1] and ref.pops([1.0, 1.5])[1].tolist() == [4, 4, 4, 4, 1]
    fe = ref.fe(ref.pops([1.5])[0])
    assert fe[0] == 0 and fe[4] == np.float32(-np.log(np.float64(np.float32(0.25))))
    nn = ref.nn(fe)
    assert nn[0].tolist() == [3, 0, 0, 0, 1] and nn[2][4] == 1 and nn[2][0] == 6
    assert ref.sigma2(nn[1]) == (0.0 + 1.0 + 1.0 + 0.0 + 41.0) / 5.0
    assert ref.pairs(1.0).tolist() == [[0, 3]] and len(ref.pairs(np.nextafter(np.float32(1.0), np.float32(2.0)))) == 5
    empty = S.Ref(probe, oracle, np.zeros((0, 3), dtype=np.float32))
    assert empty.pops([1.0]).shape == (1, 0) and np.isnan(empty.sigma2(np.zeros(0, dtype=np.float32)))
    assert [len(x) for x in empty.nn(np.zeros(0, dtype=np.float32))] == [0, 0, 0, 0]
