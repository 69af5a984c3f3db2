"""A/B of the pruned wide neighbour sweep against the unpruned one of another build of the library.

    python scratch/wide_nn_pruned_ab.py OLD_LIB [OUT_JSON]        both sides alternating in one process, 3 warm-ups, median of 5
    python scratch/wide_nn_pruned_ab.py --trace                   the new call alone, twice per shape (for a kernel trace: the
                                                                  three launches of a call are the last three wide_sweep_kernel rows)

OLD_LIB: libdcdensity.so of the commit before (its dc_hip_nearest_neighbors_wide_dev is side A); side B is
dc_hip_nearest_neighbors_wide_pruned_dev of this tree.  Kernel time: dc_hip_last_sweep_ms(1) of the library that ran the
call (the launches of a call are bracketed, the bounds kernels between them included); call: wall time of the
synchronised call; preparation = call - kernel."""
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
from clustering_amd import capi, density  # noqa: E402
from clustering_amd.synth import gaussian_blobs  # noqa: E402

PEAK_TFLOPS = 2500.0
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
NN_ARGS = [vp, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp]


def bind(path):
    lib = C.CDLL(path)
    for name in ("dc_hip_nearest_neighbors_wide_dev", "dc_hip_nearest_neighbors_wide_pruned_dev"):
        if hasattr(lib, name):
            getattr(lib, name).restype = i32
            getattr(lib, name).argtypes = NN_ARGS
    lib.dc_hip_wide_workspace_bytes.restype = sz
    lib.dc_hip_wide_workspace_bytes.argtypes = [sz, sz, sz]
    lib.dc_hip_wide_pruned_workspace_bytes.restype = sz
    lib.dc_hip_wide_pruned_workspace_bytes.argtypes = [sz, sz, sz]
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
    def __init__(self, lib, pruned, ct, ft):
        n, d = ct.shape
        self.lib, self.pruned, self.ct, self.ft, self.n, self.d = lib, pruned, ct, ft, n, d
        need = (lib.dc_hip_wide_pruned_workspace_bytes if pruned else lib.dc_hip_wide_workspace_bytes)(n, d, 1)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.out = [torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"),
                    torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")]

    def call(self):
        fn = self.lib.dc_hip_nearest_neighbors_wide_pruned_dev if self.pruned else self.lib.dc_hip_nearest_neighbors_wide_dev
        a = (0, 0) if self.pruned else (0, self.n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(p(self.ct), self.n, self.d, p(self.ft), a[0], a[1], p(self.out[0]), p(self.out[1]), p(self.out[2]), p(self.out[3]),
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


def shapes():
    """(label, coords, r) -- the free energies are those of the populations at r"""
    c = gaussian_blobs(200000, 100, seed=20240)
    yield "200000 x 100, fe from populations at r2 = 0.92", c, float(np.sqrt(0.92))
    yield "100000 x 256, fe from populations at r2 = 3.078", gaussian_blobs(100000, 256, seed=20240), float(np.sqrt(3.078))
    flat = c.copy()
    flat[:, :2] = 0.0
    yield "200000 x 100, columns 0 and 1 zeroed (one cell, nothing to prune)", flat, float(np.sqrt(0.92))


def free_energies(ct, r):
    pops = density.calculate_populations_wide_pruned(ct, [r])
    return density.calculate_free_energies(pops[0].contiguous())


def main():
    if sys.argv[1] == "--trace":
        new = bind(capi.LIB_PATH)
        for label, c, r in shapes():
            ct = torch.from_numpy(c).cuda()
            side = Side(new, True, ct, free_energies(ct, r))
            print(label, side.call(), side.call(), side.info(), flush=True)
        return
    old, new = bind(sys.argv[1]), bind(capi.LIB_PATH)
    assert not hasattr(old, "dc_hip_nearest_neighbors_wide_pruned_dev"), "OLD_LIB is to be the library of the commit before"
    results = []
    for label, c, r in shapes():
        ct = torch.from_numpy(c).cuda()
        ft = free_energies(ct, r)
        n, d = c.shape
        a, b = Side(old, False, ct, ft), Side(new, True, ct, ft)
        for _ in range(3):
            a.call()
            b.call()
        ta, tb = [], []
        for _ in range(5):
            ta.append(a.call())
            tb.append(b.call())
        equal = all(bool((x.view(torch.int32) == y.view(torch.int32)).all()) for x, y in zip(a.out, b.out))
        row = {"shape": label, "rows": n, "cols": d, "seed": 20240, "outputs_equal": equal}
        all_tiles = 16 * ((n + 127) // 128) ** 2
        for tag, side, t in (("unpruned", a, ta), ("pruned", b, tb)):
            wall, kern = statistics.median(x[0] for x in t), statistics.median(x[1] for x in t)
            tiles, mfmas, exact = side.info()
            row[tag] = {"call_ms": wall, "kernel_ms": kern, "preparation_ms": wall - kern, "tiles": tiles, "tiles_of_all": tiles / all_tiles,
                        "mfmas": mfmas, "exact_pairs": exact, "issued_tflops": mfmas * 2.0 * 32 * 32 * 16 / (kern * 1e-3) / 1e12,
                        "of_peak": mfmas * 2.0 * 32 * 32 * 16 / (kern * 1e-3) / 1e12 / PEAK_TFLOPS}
        row["speedup_call"] = row["unpruned"]["call_ms"] / row["pruned"]["call_ms"]
        row["speedup_kernel"] = row["unpruned"]["kernel_ms"] / row["pruned"]["kernel_ms"]
        print(json.dumps(row), flush=True)
        results.append(row)
        del a, b
        torch.cuda.empty_cache()
    out = {"protocol": "one MI355X, both sides alternating in one process, 3 warm-ups, median of 5; kernel time from "
                       "dc_hip_last_sweep_ms (the pruned call: its three launches and the bounds kernels between them), call = wall "
                       "time of the synchronised call, preparation = call - kernel; unpruned = dc_hip_nearest_neighbors_wide_dev of "
                       "the parent commit's library; peak = 2500 TFLOP/s of f16 MFMA",
           "results": results}
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
