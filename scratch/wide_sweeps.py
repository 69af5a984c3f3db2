"""Sweep times of the wide kernels (n_cols > 400) next to the generic kernels at 400 columns.
Run from the repository root on a GPU: python scratch/wide_sweeps.py.  Times: [fastest, slowest] of three calls; rates from
the fastest."""
import sys, time, json
import numpy as np
import torch
sys.path.insert(0, ".")
from clustering_amd import capi, density as dens
from clustering_amd.synth import gaussian_blobs


def timed(f, reps=3):
    """one warm call, then reps timed calls, each ending in a synchronise -> (fastest, slowest) in s"""
    f(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); f(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return min(ts), max(ts)


def run(n, D):
    c = gaussian_blobs(n, D, seed=7)
    ct = torch.from_numpy(c).cuda()
    r = float(np.float32(0.08 * np.sqrt(2.0 * D)))
    r2 = np.float32(r * r)
    radii = [r * 0.9, r, r * 1.1]
    pops = dens.calculate_populations_partial(ct, radii, variant="direct")
    fe = dens.calculate_free_energies(pops[1].contiguous())
    out = {}
    out["pops3"] = timed(lambda: dens.calculate_populations_partial(ct, radii, variant="direct"))
    out["nn"] = timed(lambda: dens.nearest_neighbors_partial(ct, fe, variant="direct"))
    p = torch.zeros(n, dtype=torch.int32, device="cuda"); cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    def count():
        capi.check(capi.lib.dc_hip_radius_pairs_dev(dens._dev(ct), n, D, float(r2), dens._dev(p), None, 0, dens._dev(cnt),
                                                    None, 0, dens._stream_ptr()), "pairs")
    out["pair_count"] = timed(count)
    comp = torch.arange(n, dtype=torch.int32, device="cuda")
    rank = torch.from_numpy(np.random.default_rng(1).permutation(n).astype(np.int32)).cuda()
    out["min_edge"] = timed(lambda: dens.radius_min_edge(ct, r2, comp, rank))
    pc = float(n) * n * D   # pair-columns of one sweep (the three-radius population sweep is one sweep)
    res = {"n": n, "D": D, "pairs": int(cnt.item()), "mean_pop": float(pops[1].float().mean().item())}
    for k, (t_min, t_max) in out.items():
        res[k + "_s"] = [round(t_min, 4), round(t_max, 4)]
        res[k + "_Gpc_per_s"] = round(pc / t_min / 1e9, 1)
    print(json.dumps(res), flush=True)


for n, D in [(200000, 400), (200000, 401), (100000, 1024)]:
    run(n, D)
