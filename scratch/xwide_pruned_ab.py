"""A/B of the pruned self sweeps of 257..1024 columns against the unpruned entry points of the same library
(dc_hip_*_xwide_dev: the parent commit's code).

    python scratch/xwide_pruned_ab.py SHAPE OUT_JSON     one shape per process: its population and its neighbour sweep
    python scratch/xwide_pruned_ab.py --merge OUT_JSON PART_JSON...      the parts into the record, with the library's digest

SHAPE: np512, np1024    nothing to prune: synth.gaussian_blobs, the radius of DESIGN.md 4.31's table (25 % intra-blob quantile)
       sp512, sp1024    spectrum: the same blobs with column k scaled by 1 / sqrt(1 + k) -- the shape of PCA-ordered
                        trajectories --, the radius at the 25 % intra-blob quantile of THAT data
       st1024           stretched: tests/xwidepruneref.py's data (columns 0 / 1 x 8) at its base radius
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

SHAPES = {"np512": ("plain", 100000, 512), "np1024": ("plain", 50000, 1024), "sp512": ("spectrum", 100000, 512),
          "sp1024": ("spectrum", 50000, 1024), "st1024": ("stretched", 50000, 1024)}


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
    outs = lambda o: o if isinstance(o, tuple) else (o,)
    equal = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(outs(out_a), outs(out_b)))
    row = {"outputs_equal": equal}
    for name, runs, info in (("unpruned", ta, density.xwide_sweep_info(dev)), ("pruned", tb, density.xwide_pruned_info(dev))):
        call, kern = statistics.median(x[0] for x in runs), statistics.median(x[1] for x in runs)
        tiles, mfmas, exact = info
        row[name] = {"call_ms": call, "kernel_ms": kern, "preparation_ms": call - kern, "call_ms_runs": [x[0] for x in runs],
                     "kernel_ms_runs": [x[1] for x in runs], "tiles": tiles, "mfmas": mfmas, "exact_pairs": exact,
                     "exact_share_of_evaluated_pairs": exact / (1024.0 * tiles) if tiles else None}
    row["tile_share"] = row["pruned"]["tiles"] / row["unpruned"]["tiles"]
    row["speedup_call"] = row["unpruned"]["call_ms"] / row["pruned"]["call_ms"]
    return row


def run(shape):
    kind, n, d = SHAPES[shape]
    density.sweep_timing(True)
    c, r = data(kind, n, d)
    ct = torch.from_numpy(c).cuda()
    dev = ct.device
    fe = density.calculate_free_energies(density.calculate_populations_xwide(ct, [r])[0].contiguous())
    row = {"shape": shape, "data": kind, "rows": n, "cols": d, "radius": r,
           "populations": ab("pop", lambda: density.calculate_populations_xwide(ct, [r]),
                             lambda: density.calculate_populations_xwide_pruned(ct, [r]), dev),
           "neighbours": ab("nn", lambda: density.nearest_neighbors_xwide(ct, fe),
                            lambda: density.nearest_neighbors_xwide_pruned(ct, fe), dev)}
    row["mean_population"] = float(density.calculate_populations_xwide(ct, [r]).float().mean())
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
