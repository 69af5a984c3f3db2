"""Without a GPU: every case of tests/test_gpu_pruned_edges.py is built and its conditions are checked on the referee's
data -- ties at the radius and one float inside it exist, the radii are squares of floats, at least 10 % of the queries
have tied nearest candidates at a positive d2, cross pairs sit exactly at the box gap, the component cases have their
cross pairs on the intended side of the largest radius, the far frame's lower neighbour lies at the other end, and every
case reaches the side of the statistics flag it is meant for -- so that a broken case is caught where there is no GPU."""
import sys

import numpy as np

import prunedref as P


def test_the_helper_needs_neither_torch_nor_a_gpu():
    import subprocess
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import prunedref; "
            "assert 'torch' not in sys.modules, 'prunedref imports torch'") % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_case_conditions(probe):
    assert P.check_all_case_conditions(probe) >= 40


def test_statistics_flag_restated():
    """dc_prep.hpp stats_kernel: fin = fabsf(v) <= 5e16, element-wise"""
    c = np.zeros((4, 3), dtype=np.float32)
    assert not P.self_flagged(c)
    for v, want in ((5.0e16, False), (np.nextafter(np.float32(5.0e16), np.float32(np.inf)), True), (-6e16, True),
                    (np.nan, True), (np.inf, True), (-np.inf, True), (1e15, False)):
        d = c.copy()
        d[2, 1] = v
        assert P.self_flagged(d) == want, v


def test_referees_follow_the_self_sweep_conventions(probe):
    """pop = 1 + partners (the self term whatever the radius), nn never the frame itself, ties to the lowest frame id"""
    c = np.array([[0, 0], [1, 0], [0, 1], [0, 0], [5, 5]], dtype=np.float32)
    d2x = P.off_diagonal(probe.pairwise_d2(c))
    pops = P.expect_self_pops(d2x, [0.0, 1.0, P.radius_for(np.nextafter(np.float32(1.0), np.float32(2.0))) or 1.5, P.NAN, P.INF])
    assert pops[0].tolist() == [1] * 5 and pops[3].tolist() == [1] * 5 and pops[4].tolist() == [5] * 5
    assert pops[1].tolist() == [2, 1, 1, 2, 1] and pops[2].tolist() == [4, 4, 4, 4, 1]
    fe = np.array([1, 0, 0, 1, 2], dtype=np.float32)
    nn_i, nn_d, hd_i, hd_d = P.expect_self_nn(d2x, fe)
    assert nn_i.tolist() == [3, 0, 0, 0, 1] and hd_i.tolist() == [1, 6, 6, 1, 1]
    assert nn_d[0] == 0 and hd_d[1] == P.FLT_MAX
    assert P.expect_self_pops(d2x, [1.5], 1, 3)[0].tolist() == [0, 4, 4, 0, 0]
