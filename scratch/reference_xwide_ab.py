"""A/B of the resident reference of 257..1024 columns (density.XWideReference, the assigner's path 3) against
what it replaces, on one MI355X: 3 warm-ups, the median of 5, the two sides alternating in one process; wall time of a call
between two device synchronisations.  Writes profiles/reference_xwide_ab.json.

    python scratch/reference_xwide_ab.py [--parent-lib PATH/libdcdensity.so] [--out profiles/reference_xwide_ab.json]

--parent-lib: the library of the commit before this change, loaded beside the product for the C calls of the other side
(without it the other side is the same entry points of the product, whose kernels this change left as they were).  The
Python-level sides -- assign_frames_xwide_pruned of (b), the Assigner without the flag of (d) -- run in the product library:
the code behind them is the parent's.
Data: the stretched blobs of DESIGN.md 4.33 / 4.34 (columns 0 / 1 x 8) at their base radius; the first n_q rows are the
queries, the rest the reference.
  (a) stage + populations, and stage + populations + nearest, against the parent's _cross_xwide_pruned_ calls
  (b) XWideReference.assign of a batch against assign_frames_xwide_pruned
  (c) stage + populations at r = 1e30 against the unpruned _cross_xwide_ call
  (d) one Assigner.assign on path 3 against path 2 (the direct kernels), with a reference of 20 000 rows"""
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

SHAPES = ((20000, 100000, 512), (2000, 100000, 512), (10000, 50000, 1024))
ASSIGNER_REF = 20000
WARM, REPS = 3, 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ab(sides):
    """{name: fn} -> {name: median ms, name_runs: the five}, the sides alternating"""
    for _ in range(WARM):
        for fn in sides.values():
            timed(fn)
    ms = {k: [] for k in sides}
    for _ in range(REPS):
        for k, fn in sides.items():
            ms[k].append(timed(fn))
    out = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    out["spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in ms.items()}
    names = list(sides)
    if len(names) == 2:
        out["speedup"] = round(out[names[1]] / out[names[0]], 4)
    return out


def bind(lib, name):
    f = getattr(lib, name)
    f.restype, f.argtypes = getattr(capi.lib, name).restype, getattr(capi.lib, name).argtypes
    return f


def data(n, d):
    c = gaussian_blobs(n, d, seed=7).copy()
    c[:, :2] *= np.float32(8)
    return np.ascontiguousarray(c), float(np.sqrt(2 * 0.08 * 0.08 * (d - 2) + 2 * 0.64 * 0.64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reference_xwide_ab.json"))
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    a = ap.parse_args()
    other = C.CDLL(a.parent_lib) if a.parent_lib else capi.lib
    pops_pruned = bind(other, "dc_hip_populations_cross_xwide_pruned_dev")
    nn_pruned = bind(other, "dc_hip_nearest_neighbors_cross_xwide_pruned_dev")
    pops_plain = bind(other, "dc_hip_populations_cross_xwide_dev")
    info = bind(other, "dc_hip_wide_info_dev")
    dev, dv, stream = torch.device("cuda:0"), dens._dev, dens._stream_ptr
    rows = []
    for n_q, n_r, d in (SHAPES[k] for k in a.shapes):
        c, radius = data(n_q + n_r, d)
        Q, R = torch.from_numpy(c[:n_q].copy()).to(dev), torch.from_numpy(c[n_q:].copy()).to(dev)
        states = (np.arange(n_r) % 5).astype(np.int32)
        ws_bytes = int(capi.lib.dc_hip_cross_xwide_pruned_workspace_bytes(n_q, n_r, d, 1))
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
                t0 = dens.XWideReference(R, n_q)
            t_open.append(timed(open_))
            t0.close()
        t_full = timed(lambda: dens.XWideReference(R, n_q, radius=radius, ref_states=states).close())
        ref = dens.XWideReference(R, n_q, radius=radius, ref_states=states)
        ref.stage(Q)
        fe_q = dens.calculate_free_energies_against(ref.populations([radius])[0].contiguous(), ref.max_pop)

        def parent_nn():
            capi.check(nn_pruned(dv(Q), n_q, dv(R), n_r, d, dv(fe_q), dv(ref.fe_ref), 0, n_q, dv(nn[0]), dv(nn[1]), dv(nn[2]), dv(nn[3]),
                                 dv(ws), ws_bytes, stream()), "parent neighbours")

        row = {"shape": [n_q, n_r, d], "radius": radius, "open_ms": round(statistics.median(t_open[WARM:]), 4),
               "open_with_self_sweep_ms": round(t_full, 4), "mean_population": float(ref.populations([radius]).float().mean()),
               "workspace_bytes": {"resident": int(capi.lib.dc_hip_reference_xwide_workspace_bytes(n_r, d, n_q)), "per_call": ws_bytes}}
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
                              "parent": lambda: dens.assign_frames_xwide_pruned(Q, R, radius, states, pruned_neighbours=True)})
        want = dens.assign_frames_xwide_pruned(Q, R, radius, states, pruned_neighbours=True)
        got = ref.assign(Q)
        assert all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in want if k != "max_pop"), "the two sides disagree"
        big = 1.0e30
        row["c_nothing_to_prune"] = ab({"resident": lambda: (ref.stage(Q), ref.populations([big])),
                                        "parent_unpruned": lambda: parent_pops(pops_plain, big)})
        got = ref.populations([big])
        parent_pops(pops_plain, big)
        assert torch.equal(got, out_p), "the two sides disagree"
        ref.close()
        # (d) the host assigner: path 3 against path 2, a reference of 20 000 rows (path 2 is the direct kernels)
        Rh, Qh, st = np.ascontiguousarray(c[n_q:n_q + ASSIGNER_REF]), np.ascontiguousarray(c[:n_q]), states[:ASSIGNER_REF]
        t3 = time.perf_counter()
        a3 = dens.Assigner(Rh, st, radius, n_q, xwide=True)
        t2 = time.perf_counter()
        a2 = dens.Assigner(Rh, st, radius, n_q)
        t1 = time.perf_counter()
        assert a3.path == 3 and a2.path == 2
        row["d_assigner"] = ab({"path3": lambda: a3.assign(Qh), "path2": lambda: a2.assign(Qh)})
        row["d_assigner"]["open_ms"] = {"path3": round((t2 - t3) * 1e3, 2), "path2": round((t1 - t2) * 1e3, 2)}
        o3, o2 = a3.assign(Qh), a2.assign(Qh)
        assert all(o3[k].tobytes() == o2[k].tobytes() for k in o3), "the two paths disagree"
        a3.close()
        a2.close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    doc = {"device": torch.cuda.get_device_name(0), "warmups": WARM, "repetitions": REPS, "statistic": "median, ms, wall time of the call",
           "other_side": "the library of the commit before" if a.parent_lib else "the same entry points of this library",
           "library_digest": capi.lib.dc_hip_build_digest().decode(), "rows": rows}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
