"""A/B of the matrix-core sweeps for rows of 257..1024 columns against the direct kernels of the same library.

    python scratch/xwide_ab.py SHAPE OUT_JSON     one shape per process (the caller gives every process a time limit of its own)
    python scratch/xwide_ab.py --merge OUT_JSON PART_JSON...      the parts into the record, with the library's digest

SHAPE: pop512, nn512, pop1024, nn1024, cross512 -- or pop256, the 65..256 sweep on the same data as a yardstick.
Side B is calculate_populations_xwide / nearest_neighbors_xwide / calculate_populations_against_xwide; side A the same call
with variant="direct" -- the parent commit's code, untouched.  Both sides alternate in one process, 3 warm-ups, median of 5.
The direct kernels are timed at a TENTH of the rows (of both sets in the cross shape) and scaled by 100 -- they evaluate
every pair, so their time is quadratic in the rows --; ONE full direct sweep checks that the results are bit-identical and
is reported as it was timed.  Kernel time of side B: dc_hip_last_sweep_ms; call: wall time of the synchronised call;
preparation = call - kernel.  Radius: the 25 % quantile of the intra-blob d2 of synth.gaussian_blobs, from a sample."""
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

PEAK_TFLOPS = 2500.0
SHAPES = {"pop256": ("pop", 100000, 0, 256), "pop512": ("pop", 100000, 0, 512), "nn512": ("nn", 100000, 0, 512),
          "pop1024": ("pop", 50000, 0, 1024), "nn1024": ("nn", 50000, 0, 1024), "cross512": ("cross", 100000, 20000, 512)}


def radius_for(c):
    """the 25 % quantile of the squared distances between rows of one blob, from 2 000 rows (float64)"""
    x = c[:2000].astype(np.float64)
    g = (x * x).sum(1)
    d2 = np.maximum(g[:, None] + g[None, :] - 2.0 * x @ x.T, 0.0)
    # the centres differ in columns 0 / 1 alone and lie 1.4 apart or more, sigma = 0.08: a blob is 0.7 across in that plane
    same = ((x[:, None, :2] - x[None, :, :2]) ** 2).sum(-1) < 0.49
    np.fill_diagonal(same, False)
    return float(np.sqrt(np.quantile(d2[same], 0.25)))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run(shape):
    kind, n, n_q, d = SHAPES[shape]
    density.sweep_timing(True)
    c = gaussian_blobs(n, d, seed=20240)
    r = radius_for(c)
    ct = torch.from_numpy(c).cuda()
    small = ct[: n // 10].contiguous()
    qt = q_small = None
    if kind == "cross":
        qt = torch.from_numpy(gaussian_blobs(n_q, d, seed=20241)).cuda()
        q_small = qt[: n_q // 10].contiguous()
    wide = d <= 256
    pops_b = density.calculate_populations_wide if wide else density.calculate_populations_xwide
    info_b = density.wide_sweep_info if wide else density.xwide_sweep_info
    fe = fe_small = None
    if kind == "nn":
        fe = density.calculate_free_energies(pops_b(ct, [r])[0].contiguous())
        fe_small = fe[: n // 10].contiguous()
    if kind == "pop":
        a_small = lambda: density.calculate_populations_partial(small, [r], variant="direct")
        a_full = lambda: density.calculate_populations_partial(ct, [r], variant="direct")
        b = lambda: pops_b(ct, [r])
        which, info = "pop", info_b
    elif kind == "nn":
        a_small = lambda: density.nearest_neighbors_partial(small, fe_small, variant="direct")
        a_full = lambda: density.nearest_neighbors_partial(ct, fe, variant="direct")
        b = lambda: density.nearest_neighbors_xwide(ct, fe)
        which, info = "nn", info_b
    else:
        a_small = lambda: density.calculate_populations_against(q_small, small, [r], variant="direct")
        a_full = lambda: density.calculate_populations_against(qt, ct, [r], variant="direct")
        b = lambda: density.calculate_populations_against_xwide(qt, ct, [r])
        which, info = "pop", density.xwide_against_info
    for _ in range(3):
        a_small()
        b()
    density.last_sweep_ms(which, ct.device)   # (a read closes the bracket the warm-ups opened: the next one spans one call)
    ta, tb = [], []
    for _ in range(5):
        ta.append(timed(a_small)[0])
        wall, out_b = timed(b)
        tb.append((wall, density.last_sweep_ms(which, ct.device)))
    tiles, mfmas, exact = info(ct.device)
    full_ms, out_a = timed(a_full)
    outs = lambda o: o if isinstance(o, tuple) else (o,)
    equal = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(outs(out_a), outs(out_b)))
    call, kern = statistics.median(x[0] for x in tb), statistics.median(x[1] for x in tb)
    direct_small = statistics.median(ta)
    flops = mfmas * 2.0 * 32 * 32 * 16
    row = {"shape": shape, "kind": kind, "rows": n, "queries": n_q, "cols": d, "seed": 20240, "radius": r,
           "outputs_equal": equal,
           "matrix_cores": {"call_ms": call, "kernel_ms": kern, "kernel_ms_runs": [x[1] for x in tb], "preparation_ms": call - kern,
                            "tiles": tiles, "mfmas": mfmas, "exact_pairs": exact, "exact_share_of_evaluated_pairs": exact / (1024.0 * tiles),
                            "issued_tflops": flops / (kern * 1e-3) / 1e12, "of_peak": flops / (kern * 1e-3) / 1e12 / PEAK_TFLOPS},
           "direct": {"call_ms_at_a_tenth_of_the_rows": direct_small, "call_ms_runs_at_a_tenth": ta, "call_ms_scaled_by_100": 100.0 * direct_small,
                      "call_ms_one_full_sweep": full_ms}}
    row["speedup_call_vs_scaled_direct"] = 100.0 * direct_small / call
    row["speedup_call_vs_one_full_direct_sweep"] = full_ms / call
    return row


def main():
    if sys.argv[1] == "--merge":
        parts = [json.load(open(p)) for p in sys.argv[3:]]
        out = {"protocol": "one MI355X, both sides alternating in one process per shape, 3 warm-ups, median of 5; matrix cores: "
                           "kernel time from dc_hip_last_sweep_ms, call = wall time of the synchronised call, preparation = call - "
                           "kernel; direct = variant='direct' of the same library, timed at a tenth of the rows and scaled by 100 "
                           "(quadratic in the rows), plus one full sweep for the bit-for-bit comparison; peak = 2500 TFLOP/s of f16 MFMA",
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
