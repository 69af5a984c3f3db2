"""A/B of the pruned cross sweeps of 257..1024 columns against the unpruned entry points of the same library
(dc_hip_*_cross_xwide_dev: the parent commit's code).

    python scratch/cross_xwide_pruned_ab.py SHAPE OUT_JSON     one shape per process: its population and its neighbour sweep
    python scratch/cross_xwide_pruned_ab.py --merge OUT_JSON PART_JSON...      the parts into the record, with the library's digest

SHAPE: sp512, sp1024    spectrum: synth.gaussian_blobs with column k scaled by 1 / sqrt(1 + k) -- the shape of PCA-ordered
                        trajectories --, the radius at the 25 % intra-blob quantile of that data
       st512, st1024    stretched: tests/xwidepruneref.py's data (columns 0 / 1 x 8) at its base radius
       np512, np1024    plain blobs, nothing to prune: the radius at their 25 % intra-blob quantile
512 columns: 20 000 queries against 100 000 reference frames; 1024 columns: 10 000 against 50 000.  The first n_q rows of
one generated array are the queries, the rest the reference.  The free energies of the neighbour sweep: the reference's own
populations at the radius, the queries' against the reference on the reference's scale, as assign_frames forms them.
The two sides alternate in one process, 3 warm-ups, median of 5.  Kernel time: dc_hip_last_sweep_ms; call: wall time of the
synchronised call; preparation = call - kernel."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clustering_amd import capi, density  # noqa: E402
from clustering_amd.synth import gaussian_blobs  # noqa: E402

SIZES = {512: (20000, 100000), 1024: (10000, 50000)}
SHAPES = {"sp512": ("spectrum", 512), "sp1024": ("spectrum", 1024), "st512": ("stretched", 512), "st1024": ("stretched", 1024),
          "np512": ("plain", 512), "np1024": ("plain", 1024)}


def data(kind, n, d):
    """(coords, radius)"""
    if kind == "stretched":
        c = gaussian_blobs(n, d, seed=7).copy()
        c[:, :2] *= np.float32(8)
        return np.ascontiguousarray(c), float(np.sqrt(2 * 0.08 * 0.08 * (d - 2) + 2 * 0.64 * 0.64))
    c = gaussian_blobs(n, d, seed=20240)
    # rows of one blob: the centres differ in columns 0 / 1 alone and lie 1.4 apart or more, a blob is 0.7 across there
    x = c[:2000].astype(np.float64)
    same = ((x[:, None, :2] - x[None, :, :2]) ** 2).sum(-1) < 0.49
    np.fill_diagonal(same, False)
    if kind == "spectrum":
        c = np.ascontiguousarray(c * (1.0 / np.sqrt(1.0 + np.arange(d))).astype(np.float32)[None, :])
        x = c[:2000].astype(np.float64)
    g = (x * x).sum(1)
    d2 = np.maximum(g[:, None] + g[None, :] - 2.0 * x @ x.T, 0.0)
    return c, float(np.sqrt(np.quantile(d2[same], 0.25)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def ab(which, plain, pruned, dev):
    """both sides by turns -> the row of one sweep"""
    for _ in range(3):
        plain()
        pruned()
    density.last_sweep_ms(which, dev)   # (a read closes the bracket the warm-ups opened: the next one spans one call)
    ta, tb = [], []
    for _ in range(5):
        wall, out_a = timed(plain)
        ta.append((wall, density.last_sweep_ms(which, dev)))
        wall, out_b = timed(pruned)
        tb.append((wall, density.last_sweep_ms(which, dev)))
    outs = lambda o: tuple(x for x in (o if isinstance(o, tuple) else (o,)) if x is not None)
    equal = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(outs(out_a), outs(out_b)))
    row = {"outputs_equal": equal}
    for name, runs, info in (("unpruned", ta, density.xwide_against_info(dev)), ("pruned", tb, density.xwide_against_pruned_info(dev))):
        call, kern = statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs)
        tiles, mfmas, exact = info
        row[name] = {"call_ms": call, "kernel_ms": kern, "preparation_ms": call - kern, "call_ms_runs": [x[0] for x in runs],
                     "kernel_ms_runs": [x[1] for x in runs], "tiles": tiles, "mfmas": mfmas, "exact_pairs": exact,
                     "exact_share_of_evaluated_pairs": exact / (1024.0 * tiles) if tiles else None}
    row["tile_share"] = row["pruned"]["tiles"] / row["unpruned"]["tiles"]
    row["speedup_call"] = row["unpruned"]["call_ms"] / row["pruned"]["call_ms"]
    row["speedup_kernel"] = row["unpruned"]["kernel_ms"] / row["pruned"]["kernel_ms"]
    return row


def run(shape):
    kind, d = SHAPES[shape]
    n_q, n_r = SIZES[d]
    density.sweep_timing(True)
    c, r = data(kind, n_q + n_r, d)
    q, ref = torch.from_numpy(np.ascontiguousarray(c[:n_q])).cuda(), torch.from_numpy(np.ascontiguousarray(c[n_q:])).cuda()
    dev = q.device
    pops_ref = density.calculate_populations_xwide(ref, [r])[0].contiguous()
    fe_ref = density.calculate_free_energies(pops_ref)
    pops_q = density.calculate_populations_against_xwide(q, ref, [r])[0].contiguous()
    fe_q = density.calculate_free_energies_against(pops_q, int(pops_ref.max().item()))
    row = {"shape": shape, "data": kind, "queries": n_q, "reference": n_r, "cols": d, "radius": r,
           "mean_population": float(pops_q.float().mean()),
           "populations": ab("pop", lambda: density.calculate_populations_against_xwide(q, ref, [r]),
                             lambda: density.calculate_populations_against_xwide_pruned(q, ref, [r]), dev),
           "neighbours": ab("nn", lambda: density.nearest_reference_xwide(q, ref, fe_q, fe_ref),
                            lambda: density.nearest_reference_xwide_pruned(q, ref, fe_q, fe_ref), dev),
           "neighbours_nn_only": ab("nn", lambda: density.nearest_reference_xwide(q, ref),
                                    lambda: density.nearest_reference_xwide_pruned(q, ref), dev)}
    return row


def main():
    if sys.argv[1] == "--merge":
        parts = [json.load(open(p)) for p in sys.argv[3:]]
        out = {"protocol": "one MI355X, one process per shape, the unpruned and the pruned call of the same library by turns, 3 warm-ups, "
                           "median of 5; kernel time from dc_hip_last_sweep_ms, call = wall time of the synchronised call, "
                           "preparation = call - kernel",
               "library_digest": capi.lib.dc_hip_build_digest().decode(), "results": parts}
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)
        return
    row = run(sys.argv[1])
    print(json.dumps(row), flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
