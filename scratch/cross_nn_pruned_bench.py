#!/usr/bin/env python3
"""Measurement of DESIGN 4.17's table for nearest_reference(..., pruned=True): whole calls with their preparation, HIP
events, 2 warm-ups, median of 7 with min and max, both paths in ONE process on ONE device.  The baseline is
nearest_reference(variant="mfma"), the every-pair matrix-core sweep.  Per row the pruned sweep's evaluated share of the
tile pairs and its reference shares; then whole assign_frames with and without pruned_neighbours on the assignment
shape.  Prints one JSON line per row."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clustering_amd import capi, density as dens   # noqa: E402
from clustering_amd.synth import gaussian_blobs    # noqa: E402
from cross_pruned_bench import timed               # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D, r = 10, 0.2
    blobs = gaussian_blobs(2_000_000, D)
    rng = np.random.default_rng(0)
    uni = rng.uniform(0.0, 4.0, size=(2_000_000, D)).astype(np.float32)
    shapes = [("blobs 1e6 x 1e6", blobs[0::2], blobs[1::2], True), ("uniform [0,4)^10 1e6 x 1e6", uni[:1_000_000], uni[1_000_000:], True),
              ("blobs 1e5 x 1e6", blobs[0::20], blobs[1::2], True), ("blobs 1e5 x 1e6, nn only", blobs[0::20], blobs[1::2], False)]
    digest = capi.lib.dc_hip_build_digest().decode()
    for name, Q, R, with_fe in shapes:
        q, t = torch.from_numpy(np.ascontiguousarray(Q)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda()
        fq = fr = None
        if with_fe:   # the free energies of the real pipeline: populations at r on the reference's scale
            pr = dens.calculate_populations_partial(t, [r])[0].contiguous()
            mx = int(pr.max().item())
            fr = dens.calculate_free_energies(pr)
            fq = dens.calculate_free_energies_against(dens.calculate_populations_against(q, t, [r])[0].contiguous(), mx)
        out = {"shape": name, "n_q": len(Q), "n_ref": len(R), "D": D, "digest": digest}
        res = {}
        for label, kw in (("mfma", dict(variant="mfma")), ("pruned", dict(pruned=True))):
            out[label + "_ms"] = timed(lambda: dens.nearest_reference(q, t, fq, fr, **kw))
            res[label] = dens.nearest_reference(q, t, fq, fr, **kw)
        tiles, mfma, shares = dens.evaluated_tiles_nearest_reference(dev)
        out["nn_tiles"], out["n_shares"] = tiles, shares
        out["tile_share"] = tiles / (((len(Q) + 31) // 32) * ((len(R) + 31) // 32))
        out["same"] = all(bool((a.view(torch.int32) == b.view(torch.int32)).all())
                          for a, b in zip(res["mfma"], res["pruned"]) if a is not None)
        print(json.dumps(out), flush=True)
    Q, R = blobs[0::20], blobs[1::2]
    q, t = torch.from_numpy(np.ascontiguousarray(Q)).cuda(), torch.from_numpy(np.ascontiguousarray(R)).cuda()
    states = (np.arange(len(R)) % 7 + 1).astype(np.int32)
    out = {"shape": "assign_frames blobs 1e5 x 1e6", "digest": digest}
    for label, kw in (("cross_pruned", dict(variant="cross_pruned")),
                      ("cross_pruned+pruned_neighbours", dict(variant="cross_pruned", pruned_neighbours=True))):
        out[label + "_ms"] = timed(lambda: dens.assign_frames(q, t, r, states, **kw))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
