"""A/B of a session step -- populations of one radius + free energies + neighbours -- on the pruned wide sweeps
(DC_SESSION_WIDE_SWEEPS) against the default session of the same rows, on one MI355X.

    python scratch/wide_session_ab.py OUT_JSON [--small]       (--small: 1/20 of the rows, a rehearsal of the script)

Per shape (200 000 x 100 and 100 000 x 256, gaussian blobs of seed 20240, the radii of profiles/wide_nn_pruned_ab.json):
  flag on / flag off   wall time of the three session calls (each ends in a stream synchronise), the two sessions alternating
                       in one process, 2 warm-ups, median of 5.  Flag off is the parent commit's behaviour (the direct
                       kernels); it is timed at a tenth of the rows next to a flag-on session of the same tenth, and at the
                       full rows too where the tenth, scaled by 100, stays under FULL_OFF_LIMIT_S -- the record says which.
  three _dev calls     calculate_populations_wide_pruned + calculate_free_energies + nearest_neighbors_wide_pruned on the
                       same rows, each synchronised: what a session adds on top of its sweeps (merge, copies to the host).
  preparation          a population call of a segment that owns no block of the order: the call prepares (statistics,
                       order, gathered rows, boxes, images) and sweeps nothing.  A step prepares twice, once per sweep;
                       `repeated_preparation_share` is one preparation over the flag-on step.
  one rank's share     at 2 and 8 segments: the population and the neighbour call of segment 0, the pack of its block and
                       the unpack of all blocks, each timed on its own (median of 5 after 2 warm-ups).
The outputs of the two sessions are compared at the rows both ran."""
import json
import statistics
import sys
import time

import numpy as np
import torch

import os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clustering_amd import capi, density  # noqa: E402
from clustering_amd.synth import gaussian_blobs  # noqa: E402

FULL_OFF_LIMIT_S = 6.0
SHAPES = [(200000, 100, 0.92), (100000, 256, 3.078)]     # rows, columns, squared radius


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def median_of(fn, warm=2, reps=5):
    for _ in range(warm):
        fn()
    return statistics.median(timed(fn)[0] for _ in range(reps))


def step(session, r):
    pops = session.populations([r])
    fe = session.free_energies(0)
    nn = session.nearest_neighbors()
    return pops, fe, nn


def step_times(session, r):
    """-> (ms of the populations, the free energies, the neighbours), one step"""
    a = timed(lambda: session.populations([r], fetch=False))[0]
    b = timed(lambda: session.free_energies(0, fetch=False))[0]
    c = timed(lambda: session.nearest_neighbors(nn_idx=False, nn_d2=False, hd_idx=False, hd_d2=False, sigma2=False))[0]
    return a, b, c


def ab(c, r, warm=2, reps=5):
    """flag off and flag on alternating on the same rows -> dict"""
    out = {"rows": int(c.shape[0])}
    with density.Session(c, n_devices=1, wide=False) as off, density.Session(c, n_devices=1, wide=True) as on:
        assert on.wide and not off.wide
        got_off, got_on = step(off, r), step(on, r)      # (first calls: also the comparison of the outputs)
        out["outputs_equal"] = bool((got_off[0] == got_on[0]).all() and (got_off[1].view(np.uint32) == got_on[1].view(np.uint32)).all()
                                    and all((np.asarray(x).view(np.uint32) == np.asarray(y).view(np.uint32)).all()
                                            for x, y in zip(got_off[2][:4], got_on[2][:4])) and got_off[2][4] == got_on[2][4])
        out["tiles_on"], out["tiles_off"] = on.counters(), off.counters()
        t_off, t_on = [], []
        for k in range(warm + reps):
            a, b = step_times(off, r), step_times(on, r)
            if k >= warm:
                t_off.append(a)
                t_on.append(b)
        for tag, t in (("flag_off", t_off), ("flag_on", t_on)):
            out[tag] = {"step_ms": statistics.median(sum(x) for x in t), "populations_ms": statistics.median(x[0] for x in t),
                        "free_energies_ms": statistics.median(x[1] for x in t), "neighbours_ms": statistics.median(x[2] for x in t),
                        "step_ms_min_max": [min(sum(x) for x in t), max(sum(x) for x in t)]}
    out["speedup"] = out["flag_off"]["step_ms"] / out["flag_on"]["step_ms"]
    return out


def dev_calls(ct, r):
    """the three _dev calls of a step, and a preparation alone -> dict"""
    n = ct.shape[0]
    state = {}

    def pops():
        state["pops"] = density.calculate_populations_wide_pruned(ct, [r])

    def fe():
        state["fe"] = density.calculate_free_energies(state["pops"][0].contiguous())

    def nn():
        state["nn"] = density.nearest_neighbors_wide_pruned(ct, state["fe"])

    pops(), fe()
    t = {"populations_ms": median_of(pops), "free_energies_ms": median_of(fe), "neighbours_ms": median_of(nn)}
    t["sum_ms"] = t["populations_ms"] + t["free_energies_ms"] + t["neighbours_ms"]
    blocks = (n + 127) // 128
    t["preparation_ms"] = median_of(lambda: density.calculate_populations_wide_pruned(ct, [r], blocks, blocks + 1))
    return t, state["fe"]


def rank_share(ct, ft, r, G):
    """one rank of G: segment 0's calls, its pack and the unpack of all blocks, each on its own -> dict"""
    blocks = []
    for g in range(G):
        got = density.nearest_neighbors_wide_pruned(ct, ft, g, G)
        blocks.append(density.pack_neighbor_block_wide(ct, got[0], got[1], got[2], got[3], g, G))
    flat = torch.stack(blocks).contiguous().view(-1)
    mine = density.nearest_neighbors_wide_pruned(ct, ft, 0, G)
    out = {"segments": G, "block_rows": density.neighbor_block_rows_wide(ct.shape[0], ct.shape[1], G),
           "populations_ms": median_of(lambda: density.calculate_populations_wide_pruned(ct, [r], 0, G)),
           "neighbours_ms": median_of(lambda: density.nearest_neighbors_wide_pruned(ct, ft, 0, G))}
    block = torch.empty_like(blocks[0])
    out["pack_ms"] = median_of(lambda: density.pack_neighbor_block_wide(ct, mine[0], mine[1], mine[2], mine[3], 0, G, out=block))
    res = density.unpack_neighbor_blocks_wide(ct, flat, G)
    out["unpack_ms"] = median_of(lambda: density.unpack_neighbor_blocks_wide(ct, flat, G, out=res, check=False))
    assert not density.wide_layout_status(ct.device)
    whole = density.nearest_neighbors_wide_pruned(ct, ft)
    out["unpacked_equals_whole_call"] = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(res, whole))
    out["share_ms"] = out["populations_ms"] + out["neighbours_ms"] + out["pack_ms"] + out["unpack_ms"]
    return out


def main():
    out_path = sys.argv[1]
    small = "--small" in sys.argv
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    results = []
    for n, d, r2 in SHAPES:
        if small:
            n //= 20
        r = float(np.sqrt(r2))
        c = gaussian_blobs(n, d, seed=20240)
        row = {"shape": f"{n} x {d}, one radius with r2 = {r2}", "rows": n, "cols": d, "seed": 20240}
        tenth = ab(np.ascontiguousarray(c[:n // 10]), r)
        row["at_a_tenth_of_the_rows"] = tenth
        est = tenth["flag_off"]["step_ms"] * 100.0 / 1e3
        row["flag_off_scaled_to_full_rows_s"] = est
        if est <= FULL_OFF_LIMIT_S:
            row["at_full_rows"] = ab(c, r, warm=1, reps=3)
            row["flag_off_timed_at"] = "the full rows (1 warm-up, median of 3) and a tenth of them"
        else:
            with density.Session(c, n_devices=1, wide=True) as on:
                step(on, r)
                t = [step_times(on, r) for _ in range(7)][2:]
                row["at_full_rows"] = {"rows": n, "flag_on": {"step_ms": statistics.median(sum(x) for x in t)}}
            row["flag_off_timed_at"] = "a tenth of the rows only (scaled by 100 it passes the limit of this script)"
        ct = torch.from_numpy(c).cuda()
        row["dev_calls"], ft = dev_calls(ct, r)
        on_ms = row["at_full_rows"]["flag_on"]["step_ms"]
        row["session_over_dev_calls"] = on_ms / row["dev_calls"]["sum_ms"]
        row["repeated_preparation_share"] = row["dev_calls"]["preparation_ms"] / on_ms
        row["one_rank"] = [rank_share(ct, ft, r, G) for G in (2, 8)]
        print(json.dumps(row), flush=True)
        results.append(row)
        del ct, ft
        torch.cuda.empty_cache()
    out = {"protocol": "one MI355X; wall time of synchronised calls; sessions of flag off and flag on alternating in one process, "
                       "2 warm-ups and the median of 5 unless said otherwise; flag off = dc_hip_session_open (the parent commit's "
                       "behaviour: the direct kernels at these widths)",
           "library_digest": capi.lib.dc_hip_build_digest().decode(), "small_rehearsal": small, "results": results}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
