"""A/B record of the fp32-input matrix-core sweeps for rows of 1..32 columns -> profiles/fp32_general_ab.json.

    python scratch/fp32_general_ab.py [--out profiles/fp32_general_ab.json] [--cases c3 c2 k10 k30 d5 d30]

One child process per case, each under a time limit of its own; a case that fails or runs out of time ends the script.
Inside a case the sides alternate in one process, every call synchronised: 2 warm-ups and 5 timed runs per side, the median
and the min-max spread reported.  Populations only (the sweep the roofline figure is quoted on); every side's result is
compared with the first side's before anything is timed.  Roofline: 2 D flop per pair, N^2 pairs, 157.3 TFLOP/s."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOF = 157.3e12
LIMITS = {"c3": 300, "c2": 200, "d5": 400, "d30": 600, "k10": 300, "k30": 300}


def sides_of(case, density, ct):
    fp32 = lambda radii: (lambda: density.calculate_populations_fp32(ct, radii))                                   # noqa: E731
    var = lambda v, radii: (lambda: density.calculate_populations_partial(ct, radii, variant=v))                   # noqa: E731
    if case == "c3":     # 1M x 10, one radius: the same kernel instance through both entry points
        return 1_000_000, 10, {"variant_mfma32": var("mfma32", [0.2]), "fp32_entry": fp32([0.2])}
    if case == "c2":     # 100k x 10, three radii: one sweep against a sweep per radius (the parent's way)
        radii = [0.1, 0.2, 0.3]
        return 100_000, 10, {"fp32_one_sweep_3_radii": fp32(radii),
                             "fp32_three_sweeps": lambda: [density.calculate_populations_fp32(ct, [r]) for r in radii],
                             "variant_mfma32_3_radii": var("mfma32", radii)}
    if case == "d5":
        return 1_000_000, 5, {"fp32_entry": fp32([0.15]), "variant_mfma": var("mfma", [0.15]), "variant_direct": var("direct", [0.15])}
    if case == "d30":
        eight = [0.30, 0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65]
        return 1_000_000, 30, {"fp32_entry_1_radius": fp32([0.45]), "fp32_entry_8_radii": fp32(eight),
                               "variant_mfma_1_radius": var("mfma", [0.45]), "variant_direct_1_radius": var("direct", [0.45])}
    if case in ("k10", "k30"):   # 100k rows, 2 .. 8 radii: ONE sweep against a sweep per radius, at every count
        d = int(case[1:])
        radii = [0.10, 0.15, 0.20, 0.25, 0.30, 0.35, 0.40, 0.45] if d == 10 else [0.30, 0.35, 0.40, 0.45, 0.50, 0.55, 0.60, 0.65]
        sides = {}
        for k in range(2, 9):
            sides[f"one_sweep_{k}_radii"] = fp32(radii[:k])
            sides[f"{k}_sweeps_of_one_radius"] = (lambda k=k: [density.calculate_populations_fp32(ct, [r]) for r in radii[:k]])
        return 100_000, d, sides
    raise SystemExit("unknown case " + case)


def child(case):
    import numpy as np
    import torch
    from clustering_amd import capi, density
    from clustering_amd.synth import gaussian_blobs
    shape = {"c3": (1_000_000, 10), "c2": (100_000, 10), "d5": (1_000_000, 5), "d30": (1_000_000, 30),
             "k10": (100_000, 10), "k30": (100_000, 30)}[case]
    ct = torch.from_numpy(gaussian_blobs(shape[0], shape[1], seed=20240)).cuda()
    n, d, sides = sides_of(case, density, ct)
    first = None
    for name, fn in sides.items():      # results first: every side computes the same populations
        out = fn()
        out = out if isinstance(out, torch.Tensor) else torch.cat(list(out))
        torch.cuda.synchronize()
        if first is None:
            first = out
        elif out.shape == first.shape:
            assert torch.equal(out, first), name
        elif case[0] == "k":                    # (the sides of a larger radius count: the earlier radii come first)
            assert torch.equal(out[:first.shape[0]], first), name
    times = {name: [] for name in sides}
    for rep in range(7):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    rec = {"n_rows": n, "n_cols": d, "library_digest": capi.lib.dc_hip_build_digest().decode(),
           "plan_1_radius": density.fp32_sweep_plan(n, d, 1), "sides": {}}
    for name, ts in times.items():
        ts = sorted(ts)
        rec["sides"][name] = {"ms_median": ts[2], "ms_min": ts[0], "ms_max": ts[-1], "runs_ms": ts,
                              "fraction_of_fp32_roof_one_pass": 2.0 * d * n * n / (ts[2] * 1e-3) / ROOF}
    print("RECORD " + json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp32_general_ab.json"))
    ap.add_argument("--cases", nargs="+", default=["c3", "c2", "k10", "k30", "d5", "d30"])
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    record = {"what": "fp32-input matrix-core sweeps for 1..32 columns: whole calls (statistics, order, image, sweep), "
                      "synchronised, 2 warm-ups, median of 5 per side, sides alternating in one process; "
                      "fraction_of_fp32_roof_one_pass = 2 D N^2 flop / median / 157.3 TFLOP/s (one pass of the pairs per call)",
              "cases": {}}
    for case in a.cases:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case], capture_output=True, text=True,
                           timeout=LIMITS[case])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-4000:])
            raise SystemExit(f"case {case} failed (exit {r.returncode}): nothing more is started")
        record["cases"][case] = json.loads(line[0][7:])
        print(case, json.dumps({k: round(v["ms_median"], 3) for k, v in record["cases"][case]["sides"].items()}), flush=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
