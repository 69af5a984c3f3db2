"""A/B of the radius graph and the neighbour blocks at 257..1024 columns -> profiles/xwide_graph_ab.json.

    python scratch/xwide_graph_ab.py [out.json]

One device, the calls alternating in one process, 2 warm-ups, median of 5, wall time of the whole call (preparation
included, the stream synchronised).  Per shape (100 000 x 512, 50 000 x 1024) and data (stretched blobs; blobs with
nothing to prune): a pair-count call, a first min-edge round (every frame its own component) and a whole forest, pruned
against unpruned; the direct kernel (dc_hip_radius_min_edge_dev: what these widths ran on before) against both at a TENTH
of the rows -- a round of it at the full size would pass this script's limit; and pack + unpack as a share of one rank's
neighbour call at G = 2 and 8.  The record carries the library digest."""
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
from clustering_amd import capi, density as dens   # noqa: E402
from clustering_amd.synth import gaussian_blobs    # noqa: E402

WARM, REPS = 2, 5
SHAPES = ((100000, 512), (50000, 1024))


def data(kind, n, d):
    c = gaussian_blobs(n, d, seed=7).copy()
    if kind == "stretched":
        c[:, :2] *= np.float32(8)
        r = 1.08 * np.sqrt(2 * 0.08 * 0.08 * (d - 2) + 2 * 0.64 * 0.64)
    else:
        r = np.sqrt(2 * 0.08 * 0.08 * d)
    return np.ascontiguousarray(c), float(np.float32(r) * np.float32(r))


def timed(fns):
    """the calls alternating: WARM rounds unrecorded, then REPS -> median wall ms of each"""
    ms = [[] for _ in fns]
    for rep in range(WARM + REPS):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= WARM:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return [statistics.median(m) for m in ms]


def count_call(fn, kind, ct, r2):
    n, d = ct.shape
    pops = torch.empty(n, dtype=torch.int32, device=ct.device)
    count = torch.zeros(1, dtype=torch.int64, device=ct.device)

    def call():
        ws, ws_bytes = dens._get(kind, ct.device, n, d, 1)
        capi.check(getattr(capi.lib, fn)(dens._dev(ct), n, d, r2, dens._dev(pops), None, 0, dens._dev(count), ws, ws_bytes,
                                         dens._stream_ptr()), fn)
    return call, count, pops


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "xwide_graph_ab.json")
    rec = {"protocol": f"one MI355X, the calls alternating in one process, {WARM} warm-ups, median of {REPS}, wall ms of the whole "
                       "call (preparation included); direct = dc_hip_radius_min_edge_dev, timed at a tenth of the rows together "
                       "with both matrix-core forms at that size",
           "library_digest": capi.lib.dc_hip_build_digest().decode(), "results": []}

    def save(row):
        rec["results"].append(row)
        print(json.dumps(row), flush=True)
        with open(out_path, "w") as f:
            json.dump(rec, f, indent=1)

    for n, d in SHAPES:
        for kind in ("stretched", "nothing to prune"):
            c, r2 = data(kind, n, d)
            ct = torch.from_numpy(c).cuda()
            base = {"shape": [n, d], "data": kind, "r2": r2}
            # ---- pair count ----
            plain, cnt_a, pops_a = count_call("dc_hip_radius_pairs_xwide_dev", "xwide", ct, r2)
            pruned, cnt_b, pops_b = count_call("dc_hip_radius_pairs_xwide_pruned_dev", "xwide_pruned", ct, r2)
            t = timed([plain, pruned])
            info_a, info_b = dens.xwide_sweep_info(ct.device), dens.xwide_pruned_info(ct.device)
            save(dict(base, sweep="pairs, counting only", unpruned_ms=t[0], pruned_ms=t[1], unpruned_over_pruned=t[0] / t[1],
                      outputs_equal=bool(int(cnt_a) == int(cnt_b) and torch.equal(pops_a, pops_b)), pairs=int(cnt_a),
                      unpruned_tiles=info_a[0], pruned_tiles=info_b[0], unpruned_exact=info_a[2], pruned_exact=info_b[2]))
            # ---- a first min-edge round ----
            comp = torch.arange(n, dtype=torch.int32, device=ct.device)
            rank = torch.arange(n, dtype=torch.int32, device=ct.device)
            res = {}
            t = timed([lambda: res.__setitem__("a", dens.radius_min_edge_xwide(ct, r2, comp, rank)),
                       lambda: res.__setitem__("b", dens.radius_min_edge_xwide_pruned(ct, r2, comp, rank))])
            save(dict(base, sweep="one min-edge round, every frame its own component", unpruned_ms=t[0], pruned_ms=t[1],
                      unpruned_over_pruned=t[0] / t[1],
                      outputs_equal=bool(torch.equal(res["a"][0], res["b"][0]) and torch.equal(res["a"][1], res["b"][1]))))
            # ---- ... against the direct kernel, all three at a tenth of the rows ----
            m = n // 10
            cs, comp_s, rank_s = ct[:m].contiguous(), comp[:m].contiguous(), rank[:m].contiguous()
            t = timed([lambda: res.__setitem__("d", dens.radius_min_edge(cs, r2, comp_s, rank_s)),
                       lambda: res.__setitem__("a", dens.radius_min_edge_xwide(cs, r2, comp_s, rank_s)),
                       lambda: res.__setitem__("b", dens.radius_min_edge_xwide_pruned(cs, r2, comp_s, rank_s))])
            save(dict(base, shape=[m, d], rows_are="a tenth of the shape's", sweep="one min-edge round against the direct kernel",
                      direct_ms=t[0], unpruned_ms=t[1], pruned_ms=t[2], direct_over_unpruned=t[0] / t[1], direct_over_pruned=t[0] / t[2],
                      outputs_equal=bool(torch.equal(res["d"][0], res["a"][0]) and torch.equal(res["d"][0], res["b"][0])
                                         and torch.equal(res["d"][1], res["a"][1]) and torch.equal(res["d"][1], res["b"][1]))))
            del cs
            # ---- a whole forest (host pointers: upload and the host's merges included) ----
            rank_h = np.arange(n, dtype=np.uint32)
            t = timed([lambda: res.__setitem__("fa", dens.radius_forest_xwide(c, r2, rank_h)),
                       lambda: res.__setitem__("fb", dens.radius_forest_xwide_pruned(c, r2, rank_h))])
            ka = np.sort(np.minimum(res["fa"][0][:, 0], res["fa"][0][:, 1]).astype(np.int64) * n + np.maximum(res["fa"][0][:, 0], res["fa"][0][:, 1]))
            kb = np.sort(np.minimum(res["fb"][0][:, 0], res["fb"][0][:, 1]).astype(np.int64) * n + np.maximum(res["fb"][0][:, 0], res["fb"][0][:, 1]))
            save(dict(base, sweep="forest", unpruned_ms=t[0], pruned_ms=t[1], unpruned_over_pruned=t[0] / t[1], rounds=res["fb"][1],
                      edges=int(len(kb)), outputs_equal=bool(np.array_equal(ka, kb) and res["fa"][1] == res["fb"][1])))
            # ---- pack + unpack as a share of one rank's neighbour call ----
            if kind == "stretched":
                pops = dens.calculate_populations_xwide_pruned(ct, [float(np.sqrt(r2))])
                fe = dens.calculate_free_energies(pops[0])
                if isinstance(fe, tuple):
                    fe = fe[0]
                for G in (2, 8):
                    blocks = []
                    for g in range(G - 1, -1, -1):   # (segment 0 last: its order and results stay for the timed calls)
                        got = dens.nearest_neighbors_xwide_pruned(ct, fe, g, G)
                        blocks.insert(0, dens.pack_neighbor_block_xwide(ct, got[0], got[1], got[2], got[3], g, G))
                    all_blocks = torch.stack(blocks).contiguous().view(-1)
                    outs = dens.unpack_neighbor_blocks_xwide(ct, all_blocks, G)
                    whole = dens.nearest_neighbors_xwide_pruned(ct, fe)
                    equal = all(torch.equal(a, b) for a, b in zip(outs, whole))
                    got = dens.nearest_neighbors_xwide_pruned(ct, fe, 0, G)
                    blk = torch.empty_like(blocks[0])
                    t = timed([lambda: dens.nearest_neighbors_xwide_pruned(ct, fe, 0, G),
                               lambda: dens.pack_neighbor_block_xwide(ct, got[0], got[1], got[2], got[3], 0, G, out=blk),
                               lambda: dens.unpack_neighbor_blocks_xwide(ct, all_blocks, G, out=outs, check=False)])
                    save(dict(base, sweep=f"neighbour call of rank 0 of {G}, pack, unpack", neighbour_ms=t[0], pack_ms=t[1], unpack_ms=t[2],
                              pack_and_unpack_share=(t[1] + t[2]) / t[0], outputs_equal=bool(equal),
                              refused=bool(dens.xwide_layout_status(ct.device))))
            del ct
            torch.cuda.empty_cache()
    print("written", out_path)


if __name__ == "__main__":
    main()
