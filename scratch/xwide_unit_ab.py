"""The unit map of the wide sweeps at deep K: the 8 x 8 group against smaller ones, at 257..1024 columns.

    DC_LIB_PATH=LIB python scratch/xwide_unit_ab.py time TAG SHAPE OUT_JSON   one library at one shape in a process of its own:
                                                                          3 warm-ups, 5 timed calls; the caller runs the
                                                                          libraries by turns, several rounds of processes
    python scratch/xwide_unit_ab.py merge OUT_JSON PART_JSON...           the parts into one record: per group and shape the
                                                                          median of each round, and the spread over the rounds
    DC_LIB_PATH=LIB python scratch/xwide_unit_ab.py once TAG SHAPE        two calls of one library at one shape, nothing else:
                                                                          the program a counter-only profiler run wraps
    python scratch/xwide_unit_ab.py hits DIR                              L2 hit rate of wide_sweep_kernel from the
                                                                          counter_collection.csv files under DIR, as JSON

LIB: a libdcdensity.so; the other group shapes are builds of this tree with -DDC_XWIDE_GROUP_Q=q -DDC_XWIDE_GROUP_S=s
(make CXXFLAGS_EXTRA=...).  SHAPE: pop512 (100 000 x 512) or pop1024 (50 000 x 1024), one radius at the 25 % intra-blob d2
quantile of synth.gaussian_blobs.  Kernel time: dc_hip_last_sweep_ms of the library that ran the call."""
import csv
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scratch"))

SHAPES = {"pop512": (100000, 512), "pop1024": (50000, 1024)}

def data(shape):
    import torch
    from clustering_amd.synth import gaussian_blobs
    from xwide_ab import radius_for
    n, d = SHAPES[shape]
    c = gaussian_blobs(n, d, seed=20240)
    return torch.from_numpy(c).cuda(), radius_for(c)


def main():
    mode = sys.argv[1]
    if mode == "once":
        # (the library from DC_LIB_PATH; argv[2] names it for the log)
        from clustering_amd import density
        ct, r = data(sys.argv[3])
        for _ in range(2):
            density.calculate_populations_xwide(ct, [r])
        print(sys.argv[2], sys.argv[3], density.xwide_sweep_info(ct.device), flush=True)
        return
    if mode == "hits":
        out = {}
        for root, _, files in os.walk(sys.argv[2]):
            for f in files:
                if not f.endswith("counter_collection.csv"):
                    continue
                tag = os.path.relpath(root, sys.argv[2]).split(os.sep)[0]
                acc = out.setdefault(tag, {"TCC_HIT_sum": 0.0, "TCC_MISS_sum": 0.0, "dispatches": 0})
                for row in csv.DictReader(open(os.path.join(root, f))):
                    if "wide_sweep_kernel" in row.get("Kernel_Name", "") and row.get("Counter_Name") in ("TCC_HIT_sum", "TCC_MISS_sum"):
                        acc[row["Counter_Name"]] += float(row["Counter_Value"])
                        acc["dispatches"] += row["Counter_Name"] == "TCC_HIT_sum"
        for acc in out.values():
            tot = acc["TCC_HIT_sum"] + acc["TCC_MISS_sum"]
            acc["l2_hit_rate"] = acc["TCC_HIT_sum"] / tot if tot else None
        print(json.dumps(out, indent=1))
        return
    if mode == "merge":
        parts = [json.load(open(p)) for p in sys.argv[3:]]
        groups = {}
        for q in parts:
            g = groups.setdefault((q["shape"], q["group"]), {"shape": q["shape"], "group": q["group"], "rows": q["rows"], "cols": q["cols"],
                                                             "round_medians_ms": [], "populations_sha": set(), "tiles": q["tiles"],
                                                             "mfmas": q["mfmas"], "digest": q["digest"]})
            g["round_medians_ms"].append(q["kernel_ms_median"])
            g["populations_sha"].add(q["populations_sha"])
        rows = []
        for g in groups.values():
            m = g["round_medians_ms"]
            g["kernel_ms"] = statistics.median(m)
            g["spread_ms"] = max(m) - min(m)
            g["issued_tflops"] = g["mfmas"] * 2.0 * 32 * 32 * 16 / (g["kernel_ms"] * 1e-3) / 1e12
            g["populations_sha"] = sorted(g["populations_sha"])
            rows.append(g)
        with open(sys.argv[2], "w") as f:
            json.dump({"protocol": "one MI355X; one process per (library, shape), the libraries by turns, one round after the other; "
                                   "per process 3 warm-ups and 5 timed calls, kernel time from dc_hip_last_sweep_ms; kernel_ms = the "
                                   "median of the rounds' medians, spread = largest - least of them; populations, one radius at the "
                                   "25 % intra-blob d2 quantile; populations_sha: equal across the groups of a shape",
                       "results": rows}, f, indent=1)
        return
    # time TAG SHAPE OUT_JSON, the library from DC_LIB_PATH
    import hashlib
    import torch
    from clustering_amd import capi, density
    tag, shape = sys.argv[2], sys.argv[3]
    density.sweep_timing(True)
    ct, r = data(shape)
    for _ in range(3):
        density.calculate_populations_xwide(ct, [r])
    density.last_sweep_ms("pop", ct.device)
    t = []
    for _ in range(5):
        out = density.calculate_populations_xwide(ct, [r])
        torch.cuda.synchronize()
        t.append(density.last_sweep_ms("pop", ct.device))
    tiles, mfmas, exact = density.xwide_sweep_info(ct.device)
    row = {"shape": shape, "group": tag, "rows": ct.shape[0], "cols": ct.shape[1], "radius": r, "kernel_ms_median": statistics.median(t),
           "kernel_ms_runs": t, "tiles": tiles, "mfmas": mfmas, "exact_pairs": exact,
           "populations_sha": hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:16],
           "digest": capi.lib.dc_hip_build_digest().decode(), "library": capi.LIB_PATH}
    print(json.dumps(row), flush=True)
    with open(sys.argv[4], "w") as f:
        json.dump(row, f)


if __name__ == "__main__":
    main()
