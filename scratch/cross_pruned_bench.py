#!/usr/bin/env python3
"""Measurement of DESIGN 4.17's table for variant="cross_pruned": whole calls of calculate_populations_against with
their preparation, HIP events, 2 warm-ups, median of 7, every variant in ONE process on ONE device; the pruned
sweep's evaluated share of the tile pairs from the counters of its workspace.  Prints one JSON line per shape."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clustering_amd import capi, density as dens   # noqa: E402
from clustering_amd.synth import gaussian_blobs    # noqa: E402


def timed(f, warm=2, reps=7):
    for _ in range(warm):
        f()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D, r = 10, 0.2
    blobs = gaussian_blobs(2_000_000, D)
    rng = np.random.default_rng(0)
    uni = rng.uniform(0.0, 4.0, size=(2_000_000, D)).astype(np.float32)
    shapes = [("blobs 1e6 x 1e6", blobs[0::2], blobs[1::2]), ("uniform [0,4)^10 1e6 x 1e6", uni[:1_000_000], uni[1_000_000:]),
              ("blobs 1e5 x 1e6", blobs[0::20], blobs[1::2])]
    for name, Q, R in shapes:
        q, t = torch.from_numpy(np.ascontiguousarray(Q)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda()
        out = {"shape": name, "n_q": len(Q), "n_ref": len(R), "D": D, "r": r, "digest": capi.lib.dc_hip_build_digest().decode()}
        res = {}
        for v in ("mfma", "cross_pruned"):
            buf = torch.empty((1, len(Q)), dtype=torch.int32, device=dev)
            out[v + "_ms"] = timed(lambda: dens.calculate_populations_against(q, t, [r], variant=v, out=buf))
            res[v] = buf.clone()
        tiles, mfma = dens.evaluated_tiles_against(dev)
        out["pop_tiles"] = tiles
        out["tile_share"] = tiles / (((len(Q) + 31) // 32) * ((len(R) + 31) // 32))
        out["same"] = bool((res["mfma"] == res["cross_pruned"]).all())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
