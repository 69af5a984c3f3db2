"""CPU costing of the radial gap of the neighbour sweep's ring rule, by the method of ring_cols_study.py.
C3's data (1M x 10, three blobs) in the current order -- cells of ~128 frames on columns 0/1, free energy inside the
cell, every blob a component with its centre as origin --, query groups of 6 tiles = 192 consecutive frames.  A group's
confirming radius is exact (brute force against all frames: the largest nn / lower-free-energy nn distance of its
queries).  Counted: the reference tiles a ring sweep with ideal thresholds must evaluate,
  2-D            box gap^2 in columns 0/1 < confirm
  2-D + radial   box gap^2 + gap(rho range of the tile, rho range of the group)^2 < confirm  (tiles of the group's component;
                 rho(x) = |(x - o)[2..D)|)
for free energies from the analytic mixture density and from Poisson-noised populations (mean 7 233, as C3 at r = 0.2).
Also printed: the width of a tile and of a group in rho.  Result: analytic 0.195 -> 0.181 (x 0.933), noisy 0.193 -> 0.175
(x 0.908); tiles 0.012 - 0.013 wide, groups 0.05 - 0.07; the kernel measures 0.2005 -> 0.1827 (x 0.911) at C3.
numpy only; reads nothing but the package's generator."""
import sys
import numpy as np
sys.path.insert(0, '.')
from clustering_amd.synth import gaussian_blobs

n, d, TQ, GROUPS = 1_000_000, 10, 6, 40
rng = np.random.default_rng(11)
c = gaussian_blobs(n, d)
cent = np.array([(-1.0, -0.5), (0.0, 0.5), (1.0, -0.5)], dtype=np.float32)
comp = np.argmin(((c[:, None, :2] - cent[None]) ** 2).sum(2), axis=1)
dens = np.zeros(n)
for k in range(3):
    mu = np.zeros(d, dtype=np.float32)
    mu[:2] = cent[k]
    dens += np.exp(-((c - mu) ** 2).sum(1) / (2 * 0.08 ** 2))
fe_analytic = -np.log(dens + 1e-300)
pops = 1 + rng.poisson(dens / dens.mean() * 7233.0)
fe_noisy = -np.log(pops / pops.max())
rho = np.sqrt((c[:, 2:].astype(np.float64) ** 2).sum(1))   # (the origins are the blob centres: zero behind columns 0/1)


def order_of(fe, frames_per_cell=128.0):
    lo, hi = c[:, :2].min(0), c[:, :2].max(0)
    edge = (np.prod(hi - lo) * frames_per_cell / n / 2.7) ** 0.5   # (sparse data: cells sized by the occupied area)
    idx = np.minimum(((c[:, :2] - lo) / edge).astype(np.int64), 4000)
    cell = (comp.astype(np.int64) * 4001 + idx[:, 0]) * 4001 + idx[:, 1]
    fq = ((fe - fe.min()) / (fe.max() - fe.min()) * 65535).astype(np.int64)
    return np.argsort(cell * 65536 + fq, kind='stable')


def study(name, fe):
    o = order_of(fe)
    cs, fs, rs, ks = c[o], fe[o], rho[o], comp[o]
    T = n // 32
    xy = cs[:T * 32, :2].reshape(T, 32, 2)
    lo, hi = xy.min(1), xy.max(1)
    rlo, rhi = rs[:T * 32].reshape(T, 32).min(1), rs[:T * 32].reshape(T, 32).max(1)
    tk = ks[:T * 32:32]
    sq = (cs.astype(np.float64) ** 2).sum(1)
    f2, f2r, gw = [], [], []
    for g in rng.choice(T // TQ, GROUPS, replace=False):
        t0 = g * TQ
        rows = slice(t0 * 32, (t0 + TQ) * 32)
        q, fq = cs[rows].astype(np.float64), fs[rows]
        nn, hd = np.full(192, np.inf), np.full(192, np.inf)
        for b in range(0, n, 100_000):   # (blocks: a 192 x 1M matrix of doubles at once is 1.5 GB)
            blk = slice(b, min(b + 100_000, n))
            d2 = (q * q).sum(1)[:, None] + sq[None, blk] - 2.0 * (q @ cs[blk].astype(np.float64).T)
            own = np.arange(rows.start, rows.stop) - b
            ok = (own >= 0) & (own < d2.shape[1])
            d2[np.arange(192)[ok], own[ok]] = np.inf
            nn = np.minimum(nn, d2.min(1))
            hd = np.minimum(hd, np.where(fs[None, blk] < fq[:, None], d2, np.inf).min(1))
        hd = np.where(np.isfinite(hd), hd, 0.0)   # (the free-energy minimum: nothing to confirm)
        confirm = max(nn.max(), hd.max())
        qlo, qhi = lo[t0:t0 + TQ].min(0), hi[t0:t0 + TQ].max(0)
        gap = np.maximum(0.0, np.maximum(qlo - hi, lo - qhi))
        g2 = (gap * gap).sum(1)
        glo, ghi = rlo[t0:t0 + TQ].min(), rhi[t0:t0 + TQ].max()
        gr = np.where(tk == tk[t0], np.maximum(0.0, np.maximum(rlo - ghi, glo - rhi)), 0.0)
        f2.append(float((g2 < confirm).mean()))
        f2r.append(float((g2 + gr * gr < confirm).mean()))
        gw.append(ghi - glo)
    print(f"{name:30s} 2-D rings {np.mean(f2):.3f}   2-D + radial gap {np.mean(f2r):.3f}   ratio {np.mean(f2r) / np.mean(f2):.3f}   "
          f"(tile width in rho: median {np.median(rhi - rlo):.4f}, group width: median {np.median(gw):.3f})", flush=True)


study("analytic mixture density", fe_analytic)
study("Poisson-noised populations", fe_noisy)
