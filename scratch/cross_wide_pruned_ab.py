"""A/B of the pruned wide cross population sweep against the unpruned one of another build of the library.

    python scratch/cross_wide_pruned_ab.py OLD_LIB [OUT_JSON]     both sides alternating in one process, 3 warm-ups, median of 5
    python scratch/cross_wide_pruned_ab.py --estimate             the evaluated share of the first shape from a numpy joint
                                                                  order (tests/crosswidepruneref.joint_order), no GPU

OLD_LIB: libdcdensity.so of the commit before (its dc_hip_populations_cross_wide_dev is side A); side B is
dc_hip_populations_cross_wide_pruned_dev of this tree.  Kernel time: dc_hip_last_sweep_ms(0) of the library that ran the
call; call: wall time of the synchronised call; preparation = call - kernel.  The sets: synth.gaussian_blobs(n_q + n_r, D,
seed 20240), the first n_q rows are the queries."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clustering_amd.synth import gaussian_blobs  # noqa: E402

PEAK_TFLOPS = 2500.0
vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
POP_ARGS = [vp, sz, vp, sz, sz, C.POINTER(C.c_float), sz, sz, sz, vp, vp, sz, vp]
SHAPES = (("20000 x 200000 x 100, r2 = 0.92", 20000, 200000, 100, float(np.sqrt(0.92))),
          ("20000 x 100000 x 256, r2 = 3.078", 20000, 100000, 256, float(np.sqrt(3.078))),
          ("20000 x 200000 x 100, r = 1e30 (nothing to prune)", 20000, 200000, 100, 1e30))


def sets(n_q, n_r, d):
    c = gaussian_blobs(n_q + n_r, d, seed=20240)
    return np.ascontiguousarray(c[:n_q]), np.ascontiguousarray(c[n_q:])


def estimate():
    import crosswidepruneref as ref
    label, n_q, n_r, d, r = SHAPES[0]
    Q, R = sets(n_q, n_r, d)
    perm_q, perm_r = ref.joint_order(Q, R)
    g = ref.gaps(Q, R, perm_q, perm_r)
    lo, hi = ref.pair_bounds(g, ref.launch_r2max([r])[0])
    print(json.dumps({"shape": label, "block_pairs": int(g.size), "surviving_lower": lo, "surviving_upper": hi,
                      "share_lower": lo / g.size, "share_upper": hi / g.size}))


def bind(path):
    lib = C.CDLL(path)
    for name in ("dc_hip_populations_cross_wide_dev", "dc_hip_populations_cross_wide_pruned_dev"):
        if hasattr(lib, name):
            getattr(lib, name).restype = i32
            getattr(lib, name).argtypes = POP_ARGS
    for name in ("dc_hip_cross_wide_workspace_bytes", "dc_hip_cross_wide_pruned_workspace_bytes"):
        if hasattr(lib, name):
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
    def __init__(self, lib, pruned, qt, rt, r):
        import torch
        self.lib, self.pruned, self.qt, self.rt = lib, pruned, qt, rt
        self.n_q, self.n_r, self.d = qt.shape[0], rt.shape[0], qt.shape[1]
        self.rad = (C.c_float * 1)(r)
        size = lib.dc_hip_cross_wide_pruned_workspace_bytes if pruned else lib.dc_hip_cross_wide_workspace_bytes
        self.ws = torch.empty(size(self.n_q, self.n_r, self.d, 1), dtype=torch.uint8, device="cuda")
        self.out = torch.empty((1, self.n_q), dtype=torch.int32, device="cuda")

    def call(self):
        import torch
        fn = self.lib.dc_hip_populations_cross_wide_pruned_dev if self.pruned else self.lib.dc_hip_populations_cross_wide_dev
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn(p(self.qt), self.n_q, p(self.rt), self.n_r, self.d, self.rad, 1, 0, self.n_q, p(self.out), p(self.ws),
                self.ws.numel(), None)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        ms = C.c_float(0)
        assert self.lib.dc_hip_last_sweep_ms(0, C.byref(ms)) == 0
        return wall, float(ms.value)

    def info(self):
        t, m, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert self.lib.dc_hip_wide_info_dev(p(self.ws), C.byref(t), C.byref(m), C.byref(e), None) == 0
        return int(t.value), int(m.value), int(e.value)


def main():
    if sys.argv[1] == "--estimate":
        return estimate()
    import torch
    from clustering_amd import capi
    old, new = bind(sys.argv[1]), bind(capi.LIB_PATH)
    assert not hasattr(old, "dc_hip_populations_cross_wide_pruned_dev"), "OLD_LIB is to be the library of the commit before"
    results = []
    for label, n_q, n_r, d, r in SHAPES:
        Q, R = sets(n_q, n_r, d)
        qt, rt = torch.from_numpy(Q).cuda(), torch.from_numpy(R).cuda()
        a, b = Side(old, False, qt, rt, r), Side(new, True, qt, rt, r)
        for _ in range(3):
            a.call()
            b.call()
        ta, tb = [], []
        for _ in range(5):
            ta.append(a.call())
            tb.append(b.call())
        row = {"shape": label, "queries": n_q, "references": n_r, "cols": d, "seed": 20240,
               "outputs_equal": bool((a.out == b.out).all()), "population_sum": int(b.out.sum(dtype=torch.int64))}
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
                       "dc_hip_last_sweep_ms, call = wall time of the synchronised call, preparation = call - kernel; unpruned = "
                       "dc_hip_populations_cross_wide_dev of the parent commit's library; sets: synth.gaussian_blobs(n_q + n_r, D, "
                       "seed 20240), the first n_q rows are the queries; peak = 2500 TFLOP/s of f16 MFMA",
           "results": results}
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
