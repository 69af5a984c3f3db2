"""A/B of the resident reference for rows of 1..64 columns (density.NarrowReference) against the per-call
pruned cross sweeps, on one MI355X: 3 warm-ups, the median of 5, the two sides alternating in one process; wall time of a
call between two device synchronisations.  Writes profiles/reference_ab.json.

    python scratch/reference_ab.py [--parent-lib PATH/libdcdensity.so] [--out profiles/reference_ab.json]

--parent-lib: the library of the commit before this change, loaded beside the product for the C calls of the other side
(without it the other side is the same entry points of the product, whose kernels this change left as they were).  The
Python-level side of `assign`, assign_frames(variant="cross_pruned", pruned_neighbours=True), always runs in the product
library.  Every output of the two sides is compared equal."""
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

# (name, n_q, n_r, columns, radius): the shapes DESIGN.md 4.17 measured, and one at 30 columns
SHAPES = (("blobs", 100000, 1000000, 10, 0.2), ("blobs", 2000, 1000000, 10, 0.2), ("uniform", 100000, 1000000, 10, 0.2),
          ("blobs", 100000, 1000000, 30, 0.5))
WARM, REPS = 3, 5
CROSS_PRUNED = 5


def data(kind, n, d, seed):
    if kind == "blobs":
        return gaussian_blobs(n, d, seed=seed)
    return (np.random.default_rng(seed).random((n, d), dtype=np.float32) * np.float32(4.0)).astype(np.float32)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reference_ab.json"))
    ap.add_argument("--shapes", default="0,1,2,3")
    a = ap.parse_args()
    other = C.CDLL(a.parent_lib) if a.parent_lib else capi.lib
    pops_cross = bind(other, "dc_hip_populations_cross_dev")
    nn_pruned = bind(other, "dc_hip_nearest_neighbors_cross_pruned_dev")
    nn_info = bind(other, "dc_hip_nearest_cross_pruned_info_dev")
    dev, dv, stream = torch.device("cuda:0"), dens._dev, dens._stream_ptr
    rows = []
    for k in (int(s) for s in a.shapes.split(",")):
        kind, n_q, n_r, d, radius = SHAPES[k]
        c = data(kind, n_q + n_r, d, 20240)
        Q, R = torch.from_numpy(c[:n_q].copy()).to(dev), torch.from_numpy(c[n_q:].copy()).to(dev)
        states = (np.arange(n_r) % 5).astype(np.int32)
        wp_bytes = int(capi.lib.dc_hip_cross_workspace_bytes_for(n_q, n_r, d, CROSS_PRUNED))
        wn_bytes = int(capi.lib.dc_hip_nearest_cross_pruned_workspace_bytes(n_q, n_r, d))
        wp = torch.empty(wp_bytes, dtype=torch.uint8, device=dev)
        wn = torch.empty(wn_bytes, dtype=torch.uint8, device=dev)
        out_p = torch.empty((1, n_q), dtype=torch.int32, device=dev)
        nn = [torch.empty(n_q, dtype=t, device=dev) for t in (torch.int32, torch.float32, torch.int32, torch.float32)]
        rad = (C.c_float * 1)(radius)

        def parent_pops():
            capi.check(pops_cross(dv(Q), n_q, dv(R), n_r, d, rad, 1, 0, n_q, dv(out_p), dv(wp), wp_bytes, CROSS_PRUNED, stream()),
                       "parent populations")

        def parent_pop_tiles():
            h = wp[:32].cpu().numpy().view(np.uint32)   # header words 2..3: evaluated tile pairs of the population sweep
            return int(h[2]) | (int(h[3]) << 32)

        t_open = []
        for _ in range(WARM + REPS):
            held = []
            t_open.append(timed(lambda: held.append(dens.NarrowReference(R, n_q, max_radius=radius))))
            held[0].close()
        ref = dens.NarrowReference(R, n_q, radius=radius, ref_states=states)
        ref.stage(Q)
        fe_q = dens.calculate_free_energies_against(ref.populations([radius])[0].contiguous(), ref.max_pop)

        def parent_nn():
            capi.check(nn_pruned(dv(Q), n_q, dv(R), n_r, d, dv(fe_q), dv(ref.fe_ref), 0, n_q, dv(nn[0]), dv(nn[1]), dv(nn[2]), dv(nn[3]),
                                 dv(wn), wn_bytes, stream()), "parent neighbours")

        row = {"data": kind, "shape": [n_q, n_r, d], "radius": radius, "open_ms": round(statistics.median(t_open[WARM:]), 4),
               "workspace_bytes": {"resident": int(capi.lib.dc_hip_reference_workspace_bytes(n_r, d, n_q)),
                                   "per_call_populations": wp_bytes, "per_call_neighbours": wn_bytes}}
        row["stage_alone_ms"] = ab({"stage": lambda: ref.stage(Q)})["stage"]
        row["stage_populations"] = ab({"resident": lambda: (ref.stage(Q), ref.populations([radius])), "parent": parent_pops})
        got = ref.populations([radius])
        ti = ref.info()
        parent_pops()
        assert torch.equal(got, out_p), "the two sides disagree"
        row["populations_tiles"] = {"resident": ti[0], "parent": parent_pop_tiles(), "answered": ti[3]}
        row["stage_populations_nearest"] = ab({"resident": lambda: (ref.stage(Q), ref.populations([radius]), ref.nearest(fe_q)),
                                               "parent": lambda: (parent_pops(), parent_nn())})
        got_nn = ref.nearest(fe_q)
        ni = ref.info()
        parent_nn()
        t, m, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        capi.check(nn_info(dv(wn), C.byref(t), C.byref(m), C.byref(n), stream()), "info")
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(got_nn, nn)), "the two sides disagree"
        row["nearest_tiles"] = {"resident": ni[0], "parent": int(t.value), "shares": [ni[2], int(n.value)], "answered": ni[3]}
        row["assign"] = ab({"resident": lambda: ref.assign(Q),
                            "parent": lambda: dens.assign_frames(Q, R, radius, states, variant="cross_pruned", pruned_neighbours=True)})
        x, y = ref.assign(Q), dens.assign_frames(Q, R, radius, states, variant="cross_pruned", pruned_neighbours=True)
        assert all(torch.equal(x[key].view(torch.int32), y[key].view(torch.int32)) for key in y if key != "max_pop"), "assign disagrees"
        ref.close()
        del ref, wp, wn, Q, R
        torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "warmups": WARM, "repetitions": REPS, "statistic": "median, ms, wall time of the call",
           "other_side": "the library of the commit before" if a.parent_lib else "the same entry points of this library", "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
