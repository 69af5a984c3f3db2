"""A/B of the assigner (dc_hip_assign_*, dc_hip_assigner_*) on one MI355X: 3 warm-ups, the median of 5, the
two sides alternating in one process; wall time between two device synchronisations.  Writes profiles/assign_ab.json.

    python scratch/assign_ab.py [--out profiles/assign_ab.json] [--shapes 0,1,2,3]

Per shape (batch x reference x columns, the shapes of DESIGN.md 4.28 / 4.29):
  assign_device against assign of the same handle (assign is the path of the commit before: four library calls glued
    with torch ops), for one batch and for ten batches queued back to back with one synchronisation at the end;
  density.Assigner.assign of ten batches (host pointers, chunks of one batch) with DC_ASSIGN_OVERLAP=0 against the default
    -- the switch is read once per process, so each side is a child process of this script (--overlap-child), the two
    children one after the other, each with its own warm-ups;
  the one-time cost of building the assigner on an open handle (the table of n_ref + 1 logs, its upload, the states).
Every output of the two sides is compared equal."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clustering_amd import capi, density as dens  # noqa: E402
from clustering_amd.synth import gaussian_blobs  # noqa: E402

# (n_q, n_r, columns, radius)
SHAPES = ((100000, 1000000, 10, 0.2), (2000, 1000000, 10, 0.2), (100000, 1000000, 30, 0.5), (20000, 200000, 100, float(np.sqrt(0.92))))
WARM, REPS, QUEUED = 3, 5, 10
KEYS = ("states", "pops", "fe", "nn_idx", "nn_d2", "hd_idx", "hd_d2")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab(sides):
    """{name: fn} -> {name: median ms}, the sides alternating"""
    for _ in range(WARM):
        for fn in sides.values():
            timed(fn)
    ms = {k: [] for k in sides}
    for _ in range(REPS):
        for k, fn in sides.items():
            ms[k].append(timed(fn))
    return {k: round(statistics.median(v), 4) for k, v in ms.items()}


def sets(k):
    n_q, n_r, d, radius = SHAPES[k]
    c = gaussian_blobs(n_q + n_r, d, seed=20240)
    return c[:n_q].copy(), c[n_q:].copy(), (np.arange(n_r) % 5).astype(np.int32), radius


def overlap_child(k):
    """ten batches through density.Assigner in this process's DC_ASSIGN_OVERLAP: prints the median ms and a digest"""
    import hashlib
    Q, R, states, radius = sets(k)
    many = np.ascontiguousarray(np.tile(Q, (QUEUED, 1)))
    with dens.Assigner(R, states, radius, len(Q)) as a:
        for _ in range(WARM):
            out = a.assign(many)
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            out = a.assign(many)
            ms.append((time.perf_counter() - t0) * 1e3)
        path = a.path
    digest = hashlib.sha256(b"".join(out[key].tobytes() for key in KEYS)).hexdigest()
    print(json.dumps({"ms": round(statistics.median(ms), 4), "path": path, "digest": digest}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_ab.json"))
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--overlap-child", type=int, default=None)
    a = ap.parse_args()
    if a.overlap_child is not None:
        return overlap_child(a.overlap_child)
    dev = torch.device("cuda:0")
    rows = []
    for k in (int(s) for s in a.shapes.split(",")):
        n_q, n_r, d, radius = SHAPES[k]
        Qh, Rh, states, _ = sets(k)
        Q, R = torch.from_numpy(Qh).to(dev), torch.from_numpy(Rh).to(dev)
        cls = dens.NarrowReference if d <= 64 else dens.Reference
        ref = cls(R, n_q, radius=radius, ref_states=states)
        row = {"shape": [n_q, n_r, d], "radius": round(radius, 6), "max_pop": ref.max_pop}
        # the one-time cost of the assigner on an open handle
        t_open = []
        for _ in range(WARM + REPS):
            t_open.append(timed(ref._assigner))
            capi.lib.dc_hip_assign_close(ref._assign_h)
            ref._assign_h = None
        row["assigner_open_ms"] = round(statistics.median(t_open[WARM:]), 4)
        x, y = ref.assign_device(Q), ref.assign(Q)
        assert all(torch.equal(x[key].view(torch.int32), y[key].view(torch.int32)) for key in KEYS), "the two sides disagree"
        row["answered"] = ref.info()[3]
        row["one_batch"] = ab({"assign_device": lambda: ref.assign_device(Q), "assign": lambda: ref.assign(Q)})
        row["ten_batches_queued"] = ab({"assign_device": lambda: [ref.assign_device(Q) for _ in range(QUEUED)],
                                        "assign": lambda: [ref.assign(Q) for _ in range(QUEUED)]})
        ref.close()
        del ref, Q, R, x, y
        torch.cuda.empty_cache()
        sides = {}
        for name, env in (("one_stream", {"DC_ASSIGN_OVERLAP": "0"}), ("two_streams", {})):
            base = {key: v for key, v in os.environ.items() if key != "DC_ASSIGN_OVERLAP"}
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--overlap-child", str(k)], capture_output=True, text=True,
                               timeout=900, env=dict(base, **env))
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            sides[name] = json.loads(r.stdout.strip().splitlines()[-1])
        assert sides["one_stream"]["digest"] == sides["two_streams"]["digest"], "one stream or two: the outputs differ"
        row["host_assigner_ten_batches"] = {"one_stream": sides["one_stream"]["ms"], "two_streams": sides["two_streams"]["ms"],
                                            "path": sides["two_streams"]["path"]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "library_digest": capi.lib.dc_hip_build_digest().decode(), "warmups": WARM,
           "repetitions": REPS, "statistic": "median, ms, wall time between two synchronisations", "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
