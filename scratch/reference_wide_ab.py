"""A/B of the resident reference (density.Reference) against the per-call pruned wide cross sweeps, on one
MI355X: 3 warm-ups, the median of 5, the two sides alternating in one process; wall time of a call between two device
synchronisations.  Writes profiles/reference_wide_ab.json.

    python scratch/reference_wide_ab.py [--parent-lib PATH/libdcdensity.so] [--out profiles/reference_wide_ab.json]

--parent-lib: the library of the commit before this change, loaded beside the product for the C calls of the other side
(without it the other side is the same entry points of the product, whose kernels this change left as they were).  The
Python-level side of (b), assign_frames_wide_pruned, always runs in the product library."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clustering_amd import capi, density as dens  # noqa: E402
from clustering_amd.synth import gaussian_blobs  # noqa: E402

SHAPES = ((20000, 200000, 100, 0.92), (2000, 200000, 100, 0.92), (20000, 100000, 256, 3.078))
WARM, REPS = 3, 5


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


def bind(lib, name):
    f = getattr(lib, name)
    f.restype, f.argtypes = getattr(capi.lib, name).restype, getattr(capi.lib, name).argtypes
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reference_wide_ab.json"))
    a = ap.parse_args()
    other = C.CDLL(a.parent_lib) if a.parent_lib else capi.lib
    pops_pruned = bind(other, "dc_hip_populations_cross_wide_pruned_dev")
    nn_pruned = bind(other, "dc_hip_nearest_neighbors_cross_wide_pruned_dev")
    pops_plain = bind(other, "dc_hip_populations_cross_wide_dev")
    info = bind(other, "dc_hip_wide_info_dev")
    dev, dv, stream = torch.device("cuda:0"), dens._dev, dens._stream_ptr
    rows = []
    for n_q, n_r, d, r2 in SHAPES:
        c = gaussian_blobs(n_q + n_r, d, seed=20240)
        Q, R = torch.from_numpy(c[:n_q].copy()).to(dev), torch.from_numpy(c[n_q:].copy()).to(dev)
        radius = float(np.sqrt(r2))
        states = (np.arange(n_r) % 5).astype(np.int32)
        ws_bytes = int(capi.lib.dc_hip_cross_wide_pruned_workspace_bytes(n_q, n_r, d, 1))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_p = torch.empty((1, n_q), dtype=torch.int32, device=dev)
        nn = [torch.empty(n_q, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.int32, torch.float32)]

        def parent_pops(fn=pops_pruned, r=radius):
            rad = (C.c_float * 1)(r)
            capi.check(fn(dv(Q), n_q, dv(R), n_r, d, rad, 1, 0, n_q, dv(out_p), dv(ws), ws_bytes, stream()), "parent populations")

        def parent_info():
            t, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            capi.check(info(dv(ws), C.byref(t), C.byref(m), C.byref(e), stream()), "info")
            return int(t.value), int(m.value), int(e.value)

        t_open = []
        for _ in range(WARM + REPS):
            t0 = None

            def open_():
                nonlocal t0
                t0 = dens.Reference(R, n_q)
            t_open.append(timed(open_))
            t0.close()
        ref = dens.Reference(R, n_q, radius=radius, ref_states=states)
        ref.stage(Q)
        fe_q = dens.calculate_free_energies_against(ref.populations([radius])[0].contiguous(), ref.max_pop)

        def parent_nn():
            capi.check(nn_pruned(dv(Q), n_q, dv(R), n_r, d, dv(fe_q), dv(ref.fe_ref), 0, n_q, dv(nn[0]), dv(nn[1]), dv(nn[2]), dv(nn[3]),
                                 dv(ws), ws_bytes, stream()), "parent neighbours")

        row = {"shape": [n_q, n_r, d], "r2": r2, "open_ms": round(statistics.median(t_open[WARM:]), 4),
               "workspace_bytes": {"resident": int(capi.lib.dc_hip_reference_wide_workspace_bytes(n_r, d, n_q)), "per_call": ws_bytes}}
        row["stage_alone_ms"] = ab({"stage": lambda: ref.stage(Q)})["stage"]
        row["a_populations"] = ab({"resident": lambda: (ref.stage(Q), ref.populations([radius])), "parent": parent_pops})
        got = ref.populations([radius])
        ti = ref.info()
        parent_pops()
        pi = parent_info()
        assert torch.equal(got, out_p), "the two sides disagree"
        row["populations_info"] = {"resident": {"tiles": ti[0], "exact_pairs": ti[2], "answered": ti[3]},
                                   "parent": {"tiles": pi[0], "exact_pairs": pi[2]}}
        row["a_populations_nearest"] = ab({"resident": lambda: (ref.stage(Q), ref.populations([radius]), ref.nearest(fe_q)),
                                           "parent": lambda: (parent_pops(), parent_nn())})
        got_nn = ref.nearest(fe_q)
        ni = ref.info()
        parent_nn()
        pni = parent_info()
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got_nn, nn)), "the two sides disagree"
        row["nearest_info"] = {"resident": {"tiles": ni[0], "exact_pairs": ni[2], "answered": ni[3]},
                               "parent": {"tiles": pni[0], "exact_pairs": pni[2]}}
        row["b_assign"] = ab({"resident": lambda: ref.assign(Q),
                              "parent": lambda: dens.assign_frames_wide_pruned(Q, R, radius, states, pruned_neighbours=True)})
        big = 1.0e30
        row["c_nothing_to_prune"] = ab({"resident": lambda: (ref.stage(Q), ref.populations([big])),
                                        "parent_unpruned": lambda: parent_pops(pops_plain, big)})
        ref.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "warmups": WARM, "repetitions": REPS, "statistic": "median, ms, wall time of the call",
           "other_side": "the library of the commit before" if a.parent_lib else "the same entry points of this library", "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
