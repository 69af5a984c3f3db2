"""Built cases of the pruned sweeps against a LARGE reference (tests/test_gpu_cross_pruned_big.py and its child
processes; premises: tests/test_cross_big_cases.py): more than one scan round of kListCap = 512 reference tiles, many
reference shares, every pair in the band, duplicates across rounds and the last reference the pruned kernels take
(2^24 padded positions).  Nothing here needs a GPU or torch.

The widths stand for the four classes of kernel instance (dc_mfma_kernels.hpp nm_for, kNnCoarse, kNnEarly,
kSingleBuffer, tq_pop / tq_nn):
    D =  3   NM = 1   full chains, two operand buffers, 6 query tiles per wave
    D = 10   NM = 2   kNnEarly with one coarse MFMA, 6 query tiles per wave
    D = 16   NM = 4   kNnEarly with two coarse MFMAs, 4 query tiles per wave
    D = 24   NM = 5   kSingleBuffer, 4 query tiles per wave"""
import numpy as np

import crossprunedref as cp
from crossref import F32, block_d2

CLASS_WIDTHS = [3, 10, 16, 24]
LIST_CAP = 512                       # kListCap: reference tiles of one scan round
POP_CELL, NN_CELL = 64.0, 128.0      # kPopCellFrames, kNnCellFrames
POP_TARGET, NN_TARGET = 49152, 40960  # kPopWaveTarget, kNnWaveTargetPerWave
NN_FLOOR, MAX_SHARES = 900, 64       # kNnShareFloor; the cap of pick_chunks
MAX_POS = 1 << 24                    # kPopQueueMaxRows: the longest reference order cross_pruned_takes admits


def tiles(n):
    return (n + 31) // 32


# ---- the instance classes, restated -------------------------------------------------------------------------------------
def nm_for(D):
    return (3 * D + 2 + 15) // 16


def tq_of(nm):
    """tq_pop = tq_nn"""
    return 6 if nm <= 2 else (4 if nm <= 5 else 2)


def instance_class(D):
    nm = nm_for(D)
    coarse = 1 if nm <= 2 else 2
    single = nm > 4
    early = (not single) and nm > coarse
    return "single buffer" if single else ("early, %d coarse" % coarse if early else "full chains")


# ---- the share counts, restated (pick_chunks, pop_share_floor) -----------------------------------------------------------
def pop_share_floor(T_r):
    f = T_r // 12
    return 256 if f < 256 else min(f, 1024)


def pick_chunks(T_q, tq, target, T_r, floor):
    waves = -(-T_q // tq)
    r = 1 if waves >= target else -(-target // waves)
    return max(1, min(r, min(T_r // floor, MAX_SHARES)))


def pop_shares(n_sel, n_r, D, env_floor=0):
    """shares of the population sweep for n_sel query rows; env_floor: DC_SHARE_FLOOR (0: the sweep's own)"""
    T_r = tiles(n_r)
    return pick_chunks(tiles(n_sel), tq_of(nm_for(D)), POP_TARGET, T_r, env_floor or pop_share_floor(T_r))


def nn_shares(n_sel, n_r, D, env_floor=0):
    return pick_chunks(tiles(n_sel), tq_of(nm_for(D)), NN_TARGET, tiles(n_r), env_floor or NN_FLOOR)


def round_of(pos, n_shares=1):
    """scan round in which the wave of its share meets the tile of order position pos (tile t = share + u * n_shares)"""
    return (np.asarray(pos) // 32 // n_shares) // LIST_CAP


# ---- the referee for a long reference --------------------------------------------------------------------------------------
def big_d2(probe, Q, R, chunk=2048):
    """crossref.block_d2 over R in pieces: the probe's d2 of a pair depends on its two rows alone"""
    return np.hstack([block_d2(probe, Q, R[a:a + chunk]) for a in range(0, len(R), chunk)])


# ---- the orders of the two sweeps, restated -------------------------------------------------------------------------------
def grid_keys(Q, R, frames):
    """(cell edge, keys of Q, keys of R) of the one grid (dc_prep.hpp against_grid, against_key_kernel)"""
    def col(X, k):
        return X[:, k] if X.shape[1] > k else np.zeros(len(X), np.float32)
    x, y = np.concatenate([col(Q, 0), col(R, 0)]), np.concatenate([col(Q, 1), col(R, 1)])
    lo0, lo1 = F32(x.min()), F32(y.min())
    e0, e1 = F32(x.max() - lo0), F32(y.max() - lo1)
    f = float(frames) / len(R)
    auto = np.sqrt(float(e0) * float(e1) * f) if e0 > 0 and e1 > 0 else (float(e0) + float(e1)) * f
    cell = max(F32(auto), F32(max(e0, e1) / F32(4000.0)))
    if not cell > 0:
        cell = F32(1.0)
    ny = int(min(F32(e1 / cell), F32(4000.0))) + 1

    def keys(X):
        bx = np.minimum(np.maximum((col(X, 0) - lo0) / cell, F32(0)), F32(4000)).astype(np.int64)
        by = np.minimum(np.minimum(np.maximum((col(X, 1) - lo1) / cell, F32(0)), F32(4000)).astype(np.int64), ny - 1)
        return bx * ny + np.where(bx & 1, ny - 1 - by, by)
    return cell, keys(Q), keys(R)


def cell_key_bits(n, frames):
    K = n / frames
    bound = K + 4002.0 + K / 4001.0 + 8.0
    bits = 1
    while bits < 24 and (1 << bits) < bound:
        bits += 1
    return bits


def ref_order(Q, R, frames, fe_r=None):
    """order of R: by cell, inside a cell by quantised free energy (the neighbour sweep with free energies:
    against_fe_key_kernel), then by index (a stable sort) -> (cell edge, order, position of every row)"""
    cell, key = ref_keys(Q, R, frames, fe_r)
    order = np.argsort(key, kind="stable")
    pos = np.empty(len(R), np.int64)
    pos[order] = np.arange(len(R))
    return cell, order, pos


def first_position(key, rows):
    """the lowest order position among `rows` without sorting: the row with the least (key, index) and what precedes it"""
    rows = np.asarray(rows)
    j = int(rows[np.lexsort((rows, key[rows]))[0]])
    return int((key < key[j]).sum() + (key[:j] == key[j]).sum())


def ref_keys(Q, R, frames, fe_r=None):
    """(cell edge, sort key of every reference row); the order is the stable sort by it"""
    cell, _, key = grid_keys(Q, R, frames)
    if fe_r is not None:
        cb = cell_key_bits(len(R), frames)
        fe_bits = min((24 if cb + 9 <= 24 else 32) - cb, 16)
        lo, hi = F32(fe_r.min()), F32(fe_r.max())
        span = F32(hi - lo)
        with np.errstate(invalid="ignore", divide="ignore"):
            u = ((fe_r - lo) / span).astype(np.float32) if span > 0 and np.isfinite(span) else np.zeros(len(R), np.float32)
        u = np.minimum(np.maximum(np.nan_to_num(u, nan=0.0), F32(0)), F32(1))
        key = (key << fe_bits) | (u.astype(np.float64) * float((1 << fe_bits) - 1)).astype(np.int64)
    return cell, key


# ---- case A: a line of reference rows whose order IS their index ----------------------------------------------------------
H = F32(2.0 ** -6)     # spacing of the line
A_RADII = [0.2, 0.1, 0.3]
A_SIZES = [16384, 16385, 32768, 32769]
A_LAYOUTS = {16384: ["end"], 16385: ["A2", "A3"], 32768: ["A1", "A2", "A3"], 32769: ["A3", "A3b"]}


def line(D, n_r, seed):
    """R: row p at x = (p + 0.5) H, but row 0 at 0 and the last row at n_r H, column 1 constant, the other columns small
    noise.  The common box of a query set inside [0, n_r H] is then n_r H x 0: a grid of one row of cells, edge
    frames x H (to an ulp; no row lies nearer than H / 2 to a cell boundary), so cell k holds exactly the rows
    [k frames, (k + 1) frames) and -- without free energies -- the order is the index: tile t = rows 32 t .. 32 t + 31."""
    rng = np.random.default_rng(seed)
    R = (rng.normal(size=(n_r, D)) * (0.05 / np.sqrt(D))).astype(np.float32)
    R[:, 0] = (np.arange(n_r, dtype=np.float64) + 0.5) * float(H)
    R[0, 0], R[-1, 0] = 0.0, n_r * float(H)
    R[:, 1] = F32(0.5)
    return R


def near_positions(R, lo, hi, n, rng):
    """n query rows at uniformly drawn x between the places of rows lo and hi of the line, noise like R's"""
    D, top = R.shape[1], len(R) * float(H)
    Q = (rng.normal(size=(n, D)) * (0.05 / np.sqrt(D))).astype(np.float32)
    Q[:, 0] = rng.uniform(max(0.0, (lo + 0.5) * float(H)), min(top, (hi + 0.5) * float(H)), n).astype(np.float32)
    Q[:, 1] = F32(0.5)
    return Q


def tie_pair(R, boundary):
    """The rows on both sides of the round boundary (order positions boundary - 1 and boundary) trade places and get
    equal noise columns; 32 queries midway between them, with the same noise columns, are exactly as far from both and
    farther from every other row.  Row `boundary - 1` -- the LOWER index -- now lies in the later cell, where it is the
    lowest index: first position of tile boundary / 32; row `boundary` lies in the earlier cell as its highest index:
    last position of the tile before.  -> (queries, lower index, higher index)"""
    a, b = boundary, boundary - 1
    xa, xb = R[b, 0], R[a, 0]            # row a takes the earlier place, row b the later one
    R[a], R[b] = R[b].copy(), R[b].copy()
    R[a, 0], R[b, 0] = xa, xb
    Q = np.tile(R[a], (32, 1))
    Q[:, 0] = F32((float(xa) + float(xb)) / 2.0)
    return Q, b, a


def tie_fe_across(n_q, n_r, lo, hi):
    """crossnnref.tie_fe with the two rows of tie_pair at the ends of their cells under the free-energy order as well:
    the lower index has the lowest free energy of its cell, the higher index the highest (still below the queries')"""
    fe_r = (np.arange(n_r) % 7).astype(np.float32) / F32(8.0)
    fe_r[:3] = F32(2.0)
    fe_r[lo], fe_r[hi] = F32(0.0), F32(0.875)
    return np.full(n_q, F32(1.0)), fe_r


def case_a(D, n_r, layout, seed=0):
    """-> dict(Q, R, boundary, tie=(lower, higher) or None).  boundary: the first order position of the later round.
    A1: every query more than the largest radius and more than a ring behind the boundary (partners in round two only);
    A2: the mirror image (round one only); A3 / A3b: queries over the last tile of a round and the first of the next
    (positions boundary - 40 .. boundary + 40) with the tie pair; end: n_r = 16384, the only round is exactly full and
    the queries lie on its last tiles."""
    R = line(D, n_r, seed + D + n_r)
    rng = np.random.default_rng(seed + 7 * D + n_r)
    boundary = 32 * LIST_CAP * (2 if layout == "A3b" else 1)
    tie = None
    if layout == "A1":
        Q = near_positions(R, boundary + 400, boundary + 600, 300, rng)
    elif layout == "A2":
        Q = near_positions(R, boundary - 600, boundary - 400, 300, rng)
    elif layout == "end":
        Q = near_positions(R, n_r - 100, n_r - 1, 300, rng)
    else:
        Qt, lo, hi = tie_pair(R, boundary)
        Q = np.vstack([near_positions(R, boundary - 40, boundary + 40, 268, rng), Qt])
        Q = np.ascontiguousarray(Q[rng.permutation(len(Q))])
        tie = (lo, hi)
    return dict(Q=Q, R=R, boundary=boundary, tie=tie)


def rand_fe(n_q, n_r, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.3, 1.0, n_q).astype(np.float32), rng.uniform(0, 1, n_r).astype(np.float32)


def case_a4(D, far_round, seed=4):
    """n_r = 32768, 200 queries 4000 rows before (far_round = 1) or behind (0) the round boundary, every reference row
    of higher free energy than every query except ONE, which lies 500 rows on the other side of the boundary: nn in one
    round, hd in the other.  -> (Q, R, fe_q, fe_r, special)"""
    n_r = 32768
    R = line(D, n_r, seed + D)
    rng = np.random.default_rng(seed + D + far_round)
    boundary = 32 * LIST_CAP
    at = boundary - 4000 if far_round == 1 else boundary + 4000
    Q = near_positions(R, at - 100, at + 100, 200, rng)
    special = boundary + 500 if far_round == 1 else boundary - 500
    fe_r = rng.uniform(1.0, 2.0, n_r).astype(np.float32)
    fe_r[special] = F32(0.25)
    return Q, R, np.full(len(Q), F32(0.5)), fe_r, special


# ---- case B: population shares ---------------------------------------------------------------------------------------------
B_FLOOR = 8
B_SHAPES = [(333, 4100), (333, 16400)]   # 129 tiles -> 16 shares (129 = 8 x 16 + 1); 513 tiles -> the cap of 64 shares
JOIN_FLOOR, JOIN_ROWS = 600, 40000      # 1250 tiles -> 2 shares of 625 tiles: two rounds each


# ---- case C: every pair in the band ----------------------------------------------------------------------------------------
C_SIZES = [64, 96, 2048]


def case_c(D, n_r):
    """R: n_r copies of the lattice point (4, 4) / 8 (other columns 0.5).  Q: 192 rows exactly g / 8 from it.  g = 23 of
    crossprunedref.lattice_radii is a prime 3 mod 4: the circle of radius 23 has no lattice points off the axes, so the
    queries cycle over the four axis points.  -> (Q, R, g, [r_at, r_above, r_below])"""
    g, radii = cp.lattice_radii()
    R = np.tile(cp.lattice_points([4], [4], D), (n_r, 1))
    pts = np.vstack([cp.lattice_points([4 + g], [4], D), cp.lattice_points([4 - g], [4], D),
                     cp.lattice_points([4], [4 + g], D), cp.lattice_points([4], [4 - g], D)])
    return np.ascontiguousarray(pts[np.arange(192) % 4]), R, g, radii


def c_fe(n_r, where):
    """Every reference row ties, so hd is the LOWEST INDEX of lower free energy: k0 = 5 (rows 0..4 are not lower).
    All of R lies in one cell, so with free energies its order is by free energy: the not-lower rows come last.
    where = "first" / "middle" / "last": k0 has the lowest / the median / the highest free energy of the lower rows,
    i.e. it lies in tile 0, in a middle tile, in the last tile of the order.  -> (fe_q, fe_r, k0)"""
    k0 = 5
    fe_r = np.full(n_r, F32(2.0))
    rest = np.arange(k0 + 1, n_r)
    fe_r[rest] = np.where(rest % 2 == 0, F32(0.25), F32(0.75))
    fe_r[k0] = {"first": F32(0.125), "middle": F32(0.5), "last": F32(0.875)}[where]
    return np.full(192, F32(1.0)), fe_r, k0


# ---- case D: a duplicated reference across rounds -----------------------------------------------------------------------------
def case_d(D, seed=13):
    """R: 50 distinct points x 400 copies, shuffled, 20 000 rows = 625 tiles: two rounds of one share.  Columns 0 / 1 are
    the same for every row of Q and R: one cell, every box one point, nothing pruned, and the order (without free
    energies) is the index -- the 400 copies of a point are spread over all tiles of both rounds.  Q: 150 exact copies of
    points and 150 rows near them.  -> (Q, R, point of every reference row)"""
    rng = np.random.default_rng(seed + D)
    pts = (rng.normal(size=(50, D)) * 0.3).astype(np.float32)
    pts[:, :2] = F32(0.25)
    which = rng.permutation(np.repeat(np.arange(50), 400))
    R = np.ascontiguousarray(pts[which])
    Q = pts[rng.integers(0, 50, 300)].copy()
    Q[150:, 2:] += (rng.normal(size=(150, D - 2)) * 0.02).astype(np.float32)
    return Q, R, which


# ---- case E: the last reference that is taken --------------------------------------------------------------------------------
E_SIZES = [MAX_POS, MAX_POS - 31]
E_TOP = 4096


def case_e(n_r):
    """D = 1, normal reference (the first n_r rows of one draw of 2^24), 32 queries in its sparse upper tail.  One column:
    the grid is one row of 4000 cells over the extent, the order follows x, and the partners of the queries lie at the
    end of the order.  -> (Q, R, fe_q, fe_r)"""
    rng = np.random.default_rng(24)
    R = rng.normal(size=(MAX_POS, 1)).astype(np.float32)[:n_r]
    top = np.sort(np.partition(R[:, 0], n_r - 600)[-600:])
    Q = rng.uniform(float(top[0]) + 0.1, float(top[-1]), size=(32, 1)).astype(np.float32)
    Q[:8, 0] = top[-8:]                      # exact copies of the highest rows: the very last positions
    Q[9, 0] = top[300]                       # (the query of e_radii, where the tail is still dense)
    fe_r = ((np.arange(n_r) % 1024) / 1024.0).astype(np.float32)
    fe_q = np.resize(np.array([0.0, 0.5, 2.0, np.inf, 0.125], dtype=np.float32), 32)
    return Q, R, fe_q, fe_r


def e_d2(Q, R, i):
    """numpy's float32 (q - r)^2: the canonical d2 in one column (premise: test_cross_big_cases.py)"""
    d = (Q[i, 0] - R[:, 0]).astype(np.float32)
    return (d * d).astype(np.float32)


def e_radii(Q, R):
    """a radius whose square IS the d2 of an actual pair (query 9 and its 40th nearest row), the radius above and the
    radius below it -- a pair exactly on the radius and one ulp inside it: in the guard band whatever its width -- and
    0.05.  -> ([r_below, r_at, r_above, 0.05], (query, row))"""
    from prunedref import radius_for
    cand = e_candidates(Q, R)
    d = e_d2(Q, R[cand], 9)
    for j in np.argsort(d, kind="stable")[40:400]:
        trio = [radius_for(np.nextafter(d[j], F32(0.0))), radius_for(d[j]), radius_for(np.nextafter(d[j], F32(np.inf)))]
        if all(r is not None for r in trio):
            return [float(r) for r in trio] + [0.05], (9, int(cand[j]))
    raise AssertionError("no pair distance with reachable neighbours")


def e_candidates(Q, R):
    """rows that can be a partner: a row with x <= min(q) - 1 has fl32(q - x) >= 1 for every query (1 is a float and
    rounding is monotone), so its d2 is >= 1 -- never inside a radius below 1, never nearer than a row with d2 < 1"""
    return np.flatnonzero(R[:, 0] > F32(Q[:, 0].min()) - F32(1.0))


def e_expect(Q, R, fe_q, fe_r, radii):
    """-> (populations [n_rad, n_q], [nn_idx, nn_d2, hd_idx, hd_d2], rows inside the largest radius per query), over the
    rows of e_candidates where that is proven to be the answer over all rows, else over all rows"""
    from crossref import FLT_MAX, square
    n_q, n_r = len(Q), len(R)
    pops = np.zeros((len(radii), n_q), np.int64)
    exp = [np.zeros(n_q, np.int64), np.zeros(n_q, np.float32), np.zeros(n_q, np.int64), np.zeros(n_q, np.float32)]
    inside = []
    r2 = [square(r) for r in radii]
    assert max(r2) < 1.0
    cand = e_candidates(Q, R)
    Rc, fc = R[cand], fe_r[cand]
    for i in range(n_q):
        d = e_d2(Q, Rc, i)
        for k in range(len(radii)):
            pops[k, i] = int((d < r2[k]).sum())
        inside.append(cand[d < max(r2)])
        j = int(np.argmin(d))            # (the first minimum: cand ascends, so the lowest index)
        assert d[j] < 1.0
        exp[0][i], exp[1][i] = cand[j], d[j]
        m = fc < fe_q[i]
        dm = np.where(m, d, np.inf)
        j = int(np.argmin(dm))
        if dm[j] < 1.0:
            exp[2][i], exp[3][i] = cand[j], d[j]
            continue
        m = fe_r < fe_q[i]               # no lower candidate that near: all rows decide
        if m.any():
            d = e_d2(Q, R, i)
            j = int(np.argmin(np.where(m, d, np.inf)))
            exp[2][i], exp[3][i] = j, d[j]
        else:
            exp[2][i], exp[3][i] = n_r + 1, FLT_MAX
    return pops, exp, inside
