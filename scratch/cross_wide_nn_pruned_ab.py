"""A/B of the pruned wide cross neighbour sweep against the unpruned one of another build of the library.

    python scratch/cross_wide_nn_pruned_ab.py OLD_LIB [OUT_JSON]   both sides alternating in one process, 3 warm-ups, median of 5
    python scratch/cross_wide_nn_pruned_ab.py --trace SHAPE        one warm-up and one call of the new entry point alone at shape
                                                                   0 / 1 / 2, for a kernel trace (the three launches of the call
                                                                   are the last three wide_sweep_kernel rows)

OLD_LIB: libdcdensity.so of the commit before (its dc_hip_nearest_neighbors_cross_wide_dev is side A); side B is
dc_hip_nearest_neighbors_cross_wide_pruned_dev of this tree.  Kernel time: dc_hip_last_sweep_ms(1) of the library that ran
the call (the launches of a call are bracketed, the bounds kernels between them included); call: wall time of the
synchronised call; preparation = call - kernel.  The sets: synth.gaussian_blobs(n_q + n_r, D, seed 20240), the first n_q
rows are the queries; the third shape has columns 0 and 1 zeroed (one cell, nothing to prune).  Free energies: those of the
populations at the radius named -- the reference's own, the queries' against the reference on the reference's scale."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch   # before clustering_amd.capi: the library then binds to the HIP runtime torch has loaded, one runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clustering_amd import capi, density  # noqa: E402
from clustering_amd.synth import gaussian_blobs  # noqa: E402

PEAK_TFLOPS = 2500.0
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
NN_ARGS = [vp, sz, vp, sz, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp]
SHAPES = (("20000 x 200000 x 100, r2 = 0.92", 20000, 200000, 100, float(np.sqrt(0.92)), False),
          ("20000 x 100000 x 256, r2 = 3.078", 20000, 100000, 256, float(np.sqrt(3.078)), False),
          ("20000 x 200000 x 100, r2 = 0.92, columns 0 and 1 zeroed (nothing to prune)", 20000, 200000, 100, float(np.sqrt(0.92)), True))


def sets(n_q, n_r, d, flat):
    c = gaussian_blobs(n_q + n_r, d, seed=20240)
    if flat:
        c[:, :2] = 0.0
    return np.ascontiguousarray(c[:n_q]), np.ascontiguousarray(c[n_q:])


def free_energies(qt, rt, r):
    pops_r = density.calculate_populations_wide(rt, [r])[0].contiguous()
    pops_q = density.calculate_populations_against_wide(qt, rt, [r])[0].contiguous()
    return density.calculate_free_energies_against(pops_q, int(pops_r.max().item())), density.calculate_free_energies(pops_r)


def bind(path):
    lib = C.CDLL(path)
    for name in ("dc_hip_nearest_neighbors_cross_wide_dev", "dc_hip_nearest_neighbors_cross_wide_pruned_dev"):
        if hasattr(lib, name):
            getattr(lib, name).restype = i32
            getattr(lib, name).argtypes = NN_ARGS
    for name in ("dc_hip_cross_wide_workspace_bytes", "dc_hip_cross_wide_pruned_workspace_bytes"):
        getattr(lib, name).restype = sz
        getattr(lib, name).argtypes = [sz, sz, sz, sz]
    lib.dc_hip_wide_info_dev.restype = i32
    lib.dc_hip_wide_info_dev.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
    lib.dc_hip_sweep_timing.restype = i32
    lib.dc_hip_sweep_timing.argtypes = [i32]
    lib.dc_hip_last_sweep_ms.restype = i32
    lib.dc_hip_last_sweep_ms.argtypes = [i32, C.POINTER(C.c_float)]
    lib.dc_hip_sweep_timing(1)
    return lib


def p(t):
    return C.c_void_p(t.data_ptr())


class Side:
    def __init__(self, lib, pruned, qt, rt, fq, fr):
        self.lib, self.pruned, self.qt, self.rt, self.fq, self.fr = lib, pruned, qt, rt, fq, fr
        self.n_q, self.n_r, self.d = qt.shape[0], rt.shape[0], qt.shape[1]
        size = lib.dc_hip_cross_wide_pruned_workspace_bytes if pruned else lib.dc_hip_cross_wide_workspace_bytes
        self.ws = torch.empty(size(self.n_q, self.n_r, self.d, 1), dtype=torch.uint8, device="cuda")
        self.out = [torch.empty(self.n_q, dtype=torch.int32, device="cuda") for _ in range(4)]

    def call(self):
        fn = self.lib.dc_hip_nearest_neighbors_cross_wide_pruned_dev if self.pruned else self.lib.dc_hip_nearest_neighbors_cross_wide_dev
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(p(self.qt), self.n_q, p(self.rt), self.n_r, self.d, p(self.fq), p(self.fr), 0, self.n_q, *(p(o) for o in self.out),
                p(self.ws), self.ws.numel(), None)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        ms = C.c_float(0)
        assert self.lib.dc_hip_last_sweep_ms(1, C.byref(ms)) == 0
        return wall, float(ms.value)

    def info(self):
        t, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert self.lib.dc_hip_wide_info_dev(p(self.ws), C.byref(t), C.byref(m), C.byref(e), None) == 0
        return int(t.value), int(m.value), int(e.value)


def trace(k):
    label, n_q, n_r, d, r, flat = SHAPES[k]
    Q, R = sets(n_q, n_r, d, flat)
    qt, rt = torch.from_numpy(Q).cuda(), torch.from_numpy(R).cuda()
    fq, fr = free_energies(qt, rt, r)
    b = Side(bind(capi.LIB_PATH), True, qt, rt, fq, fr)
    b.call()
    print(json.dumps({"shape": label, "call_ms, kernel_ms": b.call(), "info": b.info()}))


def main():
    if sys.argv[1] == "--trace":
        return trace(int(sys.argv[2]))
    old, new = bind(sys.argv[1]), bind(capi.LIB_PATH)
    assert not hasattr(old, "dc_hip_nearest_neighbors_cross_wide_pruned_dev"), "OLD_LIB is to be the library of the commit before"
    results = []
    for label, n_q, n_r, d, r, flat in SHAPES:
        Q, R = sets(n_q, n_r, d, flat)
        qt, rt = torch.from_numpy(Q).cuda(), torch.from_numpy(R).cuda()
        fq, fr = free_energies(qt, rt, r)
        a, b = Side(old, False, qt, rt, fq, fr), Side(new, True, qt, rt, fq, fr)
        for _ in range(3):
            a.call()
            b.call()
        ta, tb = [], []
        for _ in range(5):
            ta.append(a.call())
            tb.append(b.call())
        row = {"shape": label, "queries": n_q, "references": n_r, "cols": d, "seed": 20240,
               "outputs_equal": all(bool((x == y).all()) for x, y in zip(a.out, b.out)),
               "queries_with_a_lower_reference": int((b.out[2] != n_r + 1).sum())}
        all_tiles = 16 * ((n_q + 127) // 128) * ((n_r + 127) // 128)
        for tag, side, t in (("unpruned", a, ta), ("pruned", b, tb)):
            wall, kern = statistics.median(x[0] for x in t), statistics.median(x[1] for x in t)
            tiles, mfmas, exact = side.info()
            flops = mfmas * 2.0 * 32 * 32 * 16
            row[tag] = {"call_ms": wall, "kernel_ms": kern, "preparation_ms": wall - kern, "tiles": tiles, "tiles_of_all": tiles / all_tiles,
                        "mfmas": mfmas, "exact_pairs": exact, "issued_tflops": flops / (kern * 1e-3) / 1e12,
                        "of_peak": flops / (kern * 1e-3) / 1e12 / PEAK_TFLOPS, "workspace_bytes": side.ws.numel(),
                        "calls_ms": [x[0] for x in t], "kernels_ms": [x[1] for x in t]}
        row["speedup_call"] = row["unpruned"]["call_ms"] / row["pruned"]["call_ms"]
        row["speedup_kernel"] = row["unpruned"]["kernel_ms"] / row["pruned"]["kernel_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)
        del a, b
        torch.cuda.empty_cache()
    out = {"protocol": "one MI355X, both sides alternating in one process, 3 warm-ups, median of 5; kernel time from "
                       "dc_hip_last_sweep_ms (the pruned call: its launches and the bounds kernels between them), call = wall time of "
                       "the synchronised call, preparation = call - kernel; unpruned = dc_hip_nearest_neighbors_cross_wide_dev of the "
                       "parent commit's library; sets: synth.gaussian_blobs(n_q + n_r, D, seed 20240), the first n_q rows are the "
                       "queries; free energies of the populations at the radius named; peak = 2500 TFLOP/s of f16 MFMA",
           "results": results}
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
