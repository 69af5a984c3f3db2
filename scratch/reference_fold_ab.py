"""Parent library against branch library through the project's own A/B scripts (scratch/reference_ab.py,
scratch/reference_wide_ab.py, scratch/assign_ab.py), each run a process of its own, the two sides alternating round by
round in one session.  The parent side is the parent commit's scripts, binding and library (a built checkout of it:
clustering_amd/ with lib/libdcdensity.so, and scratch/); the branch side this tree's.  Wrote profiles/reference_fold_ab.json.

    python scratch/reference_fold_ab.py PARENT_TREE ROUNDS SECONDS [OUT.json]

SECONDS: no further round is begun (after the third) once the rounds so far suggest the next would end beyond it."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ("reference_ab", "reference_wide_ab", "assign_ab")
# script -> {metric: path in a row}; the first is the per-batch time the requirement speaks of
METRICS = {"reference_ab": {"stage_populations_nearest_ms": ("stage_populations_nearest", "resident"),
                            "stage_populations_ms": ("stage_populations", "resident"), "stage_alone_ms": ("stage_alone_ms",),
                            "assign_ms": ("assign", "resident"), "open_ms": ("open_ms",)},
           "reference_wide_ab": {"stage_populations_nearest_ms": ("a_populations_nearest", "resident"),
                                 "stage_populations_ms": ("a_populations", "resident"), "stage_alone_ms": ("stage_alone_ms",),
                                 "assign_ms": ("b_assign", "resident"), "open_ms": ("open_ms",)},
           "assign_ab": {"assign_device_one_batch_ms": ("one_batch", "assign_device"),
                         "assign_device_ten_batches_ms": ("ten_batches_queued", "assign_device"),
                         "host_assigner_ten_batches_ms": ("host_assigner_ten_batches", "two_streams"),
                         "assigner_open_ms": ("assigner_open_ms",)}}


def main():
    TREES = {"parent": os.path.abspath(sys.argv[1]), "branch": ROOT}
    rounds, budget = int(sys.argv[2]), float(sys.argv[3])
    final = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "reference_fold_ab.json")
    OUT = tempfile.mkdtemp(prefix="reference_fold_ab_")
    t0 = time.time()
    runs = {s: {side: [] for side in TREES} for s in SCRIPTS}
    done = 0
    for r in range(rounds):
        if r >= 3 and time.time() - t0 > budget * r / (r + 1):
            break
        for side, tree in TREES.items():
            for s in SCRIPTS:
                out = os.path.join(OUT, f"{side}_{s}_{r}.json")
                env = {k: v for k, v in os.environ.items() if k not in ("DC_LIB_PATH", "DC_ASSIGN_OVERLAP")}
                p = subprocess.run([sys.executable, os.path.join(tree, "scratch", s + ".py"), "--out", out], cwd=tree, env=env,
                                   capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    print(f"{side} {s} round {r}: exit status {p.returncode}\n{p.stdout[-1500:]}\n{p.stderr[-3000:]}")
                    sys.exit(1)
                runs[s][side].append(json.load(open(out))["rows"])
        done = r + 1
        print(f"round {r} done at {time.time() - t0:.0f} s", flush=True)
    doc = {"what": "the resident reference handles and the assigner before and after the two handles were folded onto one struct "
                   "and one body per step: the library, binding and scripts of the commit before (parent) against this "
                   "commit's (branch)",
           "method": "scratch/reference_ab.py, scratch/reference_wide_ab.py and scratch/assign_ab.py (3 warm-ups, the median of 5, "
                     "wall time between two device synchronisations), each run a process of its own; the two sides alternate "
                     f"round by round in one session, {done} rounds a side.  Per shape and metric: every run's median, the median "
                     "of those per side, and the parent's run-to-run spread (largest minus smallest of its runs).  ok: the "
                     "branch's median is not above the parent's by more than that spread",
           "rounds": done, "scripts": {}}
    worst = True
    for s in SCRIPTS:
        shapes = []
        for k, row in enumerate(runs[s]["branch"][0]):
            entry = {"shape": row["shape"], **({"data": row["data"]} if "data" in row else {}), "metrics": {}}
            for name, path in METRICS[s].items():
                def val(rows):
                    v = rows[k]
                    for key in path:
                        v = v[key]
                    return v
                par, br = [val(x) for x in runs[s]["parent"]], [val(x) for x in runs[s]["branch"]]
                spread = round(max(par) - min(par), 4)
                mp, mb = round(statistics.median(par), 4), round(statistics.median(br), 4)
                ok = mb <= mp + spread
                entry["metrics"][name] = {"parent_runs": par, "branch_runs": br, "parent_median": mp, "branch_median": mb,
                                          "parent_spread": spread, "ok": ok}
                worst = worst and ok
            shapes.append(entry)
        doc["scripts"][s] = shapes
    doc["all_ok"] = worst
    with open(final, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("all ok" if worst else "SOME METRIC ABOVE THE PARENT'S SPREAD")
    for s in SCRIPTS:
        for e in doc["scripts"][s]:
            first = next(iter(METRICS[s]))
            m = e["metrics"][first]
            print(s, e["shape"], first, "parent", m["parent_median"], "branch", m["branch_median"], "spread", m["parent_spread"], m["ok"])


if __name__ == "__main__":
    main()
