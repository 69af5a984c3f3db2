"""Case generators and block-pair bounds of the pruned wide population sweep's tests (65..256 columns):
tests/test_wide_pruned_cases.py checks their premises on the CPU with a numpy cell order, tests/test_gpu_wide_pruned.py
runs them on the device and takes the order from the device (density.wide_pruned_order).

The pruning check is a condition on the counters, not a measurement: with the boxes of the blocks (128 positions of the
order) formed in float64 from the coordinates, every launch evaluates the block pairs with box gap^2 < r2max -- the
survivor rule keeps them -- and none with gap^2 >= 1.001 r2max: its margin is 1.0001 and its roundings a few 2^-24."""
import functools

import numpy as np

import wideref

F32 = np.float32
BLOCK = 128          # positions per block of the order
LAUNCH_RADII = 8     # radii per launch
MARGIN_RADIUS = 3.0


def stretched(n_rows, n_cols, seed=7):
    """wideref.blobs with columns 0 and 1 multiplied by 4: the blobs lie 4 apart, 0.32 wide in the plane of the order"""
    c = wideref.blobs(n_rows, n_cols, seed=seed).copy()
    c[:, 0] *= F32(4)
    c[:, 1] *= F32(4)
    return np.ascontiguousarray(c)


def radii_for(n_cols, k=3):
    """k radii around the intra-blob distance of the stretched blobs, not sorted"""
    base = float(np.sqrt(2 * 0.08 * 0.08 * (n_cols - 2) + 2 * 0.32 * 0.32))
    return [base * f for f in (1.0, 0.9, 1.08, 0.95, 1.2, 0.8, 1.02, 0.85)[:k]]


def cell_order(c, frames_per_cell=BLOCK):
    """a spatial order as the device builds it, in numpy: cells on columns 0 / 1 with about a block's worth of frames per
    cell of the bounding box, numbered column by column in serpentine order, one stable sort.  position -> row"""
    x, y = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)
    fx, fy = np.isfinite(x), np.isfinite(y)
    lo0, hi0 = (x[fx].min(), x[fx].max()) if fx.any() else (0.0, 0.0)
    lo1, hi1 = (y[fy].min(), y[fy].max()) if fy.any() else (0.0, 0.0)
    e0, e1 = hi0 - lo0, hi1 - lo1
    f = frames_per_cell / max(len(c), 1)
    cell = np.sqrt(e0 * e1 * f) if e0 > 0 and e1 > 0 else (e0 + e1) * f
    cell = max(cell, max(e0, e1) / 4000.0)
    if not cell > 0:
        cell = 1.0
    ny = int(min(e1 / cell, 4000.0)) + 1
    ok = fx & fy
    bx = np.clip(np.where(ok, (x - lo0) / cell, 0.0), 0.0, 4000.0).astype(np.int64)
    by = np.minimum(np.clip(np.where(ok, (y - lo1) / cell, 0.0), 0.0, 4000.0).astype(np.int64), ny - 1)
    key = np.where(ok, bx * ny + np.where(bx & 1, ny - 1 - by, by), 0)
    return np.argsort(key, kind="stable")


def n_blocks(n_rows):
    return (n_rows + BLOCK - 1) // BLOCK


def block_boxes(c, perm):
    """float64 [blocks][4] = (lo0, hi0, lo1, hi1) of the rows perm[128 b .. 128 b + 127]"""
    perm = np.asarray(perm, dtype=np.int64)
    xy = c[perm][:, :2].astype(np.float64)
    out = np.empty((n_blocks(len(perm)), 4))
    for b in range(len(out)):
        p = xy[BLOCK * b:BLOCK * (b + 1)]
        out[b] = (p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max())
    return out


def box_gap2(boxes_q, boxes_r):
    """float64 [q][r]: the squared distance of the boxes in the plane"""
    q, r = boxes_q[:, None, :], boxes_r[None, :, :]
    dx = np.maximum(0.0, np.maximum(q[..., 0] - r[..., 1], r[..., 0] - q[..., 1]))
    dy = np.maximum(0.0, np.maximum(q[..., 2] - r[..., 3], r[..., 2] - q[..., 3]))
    return dx * dx + dy * dy


def pair_bounds(boxes, r2max, query_blocks=None):
    """(#{gap^2 < r2max}, #{gap^2 < 1.001 r2max}) over the (query block, reference block) pairs of the given query blocks"""
    q = boxes if query_blocks is None else boxes[np.asarray(list(query_blocks), dtype=np.int64)]
    if len(q) == 0:
        return 0, 0
    g = box_gap2(q, boxes)
    return int((g < r2max).sum()), int((g < 1.001 * r2max).sum())


def launch_r2max(radii):
    """the largest fl32(r^2) of every launch of a call (8 radii each; a NaN square counts as 0), as float64"""
    out = []
    for k in range(0, len(radii), LAUNCH_RADII):
        with np.errstate(over="ignore", invalid="ignore"):
            r2 = [F32(r) * F32(r) for r in radii[k:k + LAUNCH_RADII]]
        out.append(float(max([0.0] + [float(v) for v in r2 if v == v])))
    return out


def segment_blocks(n_rows, segment, n_segments):
    """the query blocks of a call: all of them (n_segments == 0) or segment, segment + n_segments, ..."""
    nb = n_blocks(n_rows)
    return range(nb) if n_segments == 0 else range(segment, nb, n_segments)


def tile_bounds(c, perm, radii, segment=0, n_segments=0):
    """(lower, upper) for the `tiles` counter of a call: 16 tile pairs per evaluated block pair, added over its launches"""
    boxes = block_boxes(c, perm)
    qb = segment_blocks(len(c), segment, n_segments)
    lo = hi = 0
    for r2 in launch_r2max(radii):
        a, b = pair_bounds(boxes, r2, qb)
        lo, hi = lo + 16 * a, hi + 16 * b
    return lo, hi


def shares(blocks):
    """reference shares of a launch over that many blocks (wide_shares, dc_mfma_wide_kernels.hpp): share y owns the
    blocks y, y + shares, ..."""
    s = 1
    while 2 * s <= 64 and 2 * s * 8 <= blocks:
        s *= 2
    return s


def empty_units(c, perm, r2max):
    """(units without a block pair of gap^2 < 1.001 r2max, all units): a unit is (query block, reference share), the work
    of one workgroup -- such a unit has no survivor whatever the roundings of the device's rule"""
    boxes = block_boxes(c, perm)
    near = box_gap2(boxes, boxes) < 1.001 * r2max
    sy = shares(len(boxes))
    per_unit = np.array([[near[q, y::sy].sum() for y in range(sy)] for q in range(len(boxes))])
    return int((per_unit == 0).sum()), per_unit.size


# rows x columns -> (surviving block pairs, all block pairs) of the stretched blobs under a numpy cell order, at the
# largest of radii_for(D, 3) -- the same for gap^2 < r2max and for gap^2 < 1.001 r2max
STRETCHED_TABLE = {(700, 100): (20, 36), (1500, 100): (64, 144), (2100, 100): (119, 289), (8320, 80): (1495, 4225)}


@functools.lru_cache(maxsize=None)
def margin_case(n_cols=80, seed=3):
    """-> (coords, r, rows): 256 rows in two groups of 128 that the order puts into one block each.
    Group A: column 0 <= 0, one row a at (0, 0).  Group B: column 0 >= 3 - 2^-22 with d at (3 - 2^-22, 0), b at (3, 0),
    c at (3, 2^-10), the rest further out.  a, b, c, d are equal in every other column (wideref.boundary_case's
    construction), so d2(a, d) = 9 - ulp, d2(a, b) = 9 = fl32(r * r), d2(a, c) = 9 + ulp in every summation order -- and
    the box gap of the two blocks IS the distance of (a, d), the pair one ulp inside the radius.  rows = (a, b, c, d)."""
    from clustering_amd.synth import gaussian_blobs
    n = 2 * BLOCK
    c = gaussian_blobs(n, n_cols, seed=seed, sigma=0.3)
    rng = np.random.default_rng(seed + 1)
    grp_a = np.arange(0, n, 2)            # (interleaved: the order has to sort them)
    grp_b = np.arange(1, n, 2)
    c[grp_a, 0] = rng.uniform(-4.0, -0.5, BLOCK).astype(F32)
    c[grp_b, 0] = rng.uniform(3.5, 7.0, BLOCK).astype(F32)
    c[:, 1] = rng.uniform(-0.5, 0.5, n).astype(F32)
    a, b, cc, d = int(grp_a[17]), int(grp_b[5]), int(grp_b[40]), int(grp_b[77])
    base = c[a].copy()
    base[0], base[1] = 0.0, 0.0
    for r in (a, b, cc, d):
        c[r] = base
    c[b, 0] = F32(3.0)
    c[cc, 0], c[cc, 1] = F32(3.0), F32(2.0 ** -10)
    c[d, 0] = F32(3.0) - F32(2.0 ** -22)
    return np.ascontiguousarray(c), MARGIN_RADIUS, (a, b, cc, d)


def edge_radii(n_cols=80):
    """the eight radii of test_gpu_wide_mfma.test_radii_in_any_order_and_at_the_edges and the eleven that follow them"""
    base = float(np.sqrt(2 * 0.3 * 0.3 * n_cols))
    r_edge = MARGIN_RADIUS
    eight = [base, 1e30, 0.0, r_edge, 1e-3, base * 0.8, float(np.nextafter(F32(r_edge), F32(4))), base * 1.3]
    return eight, eight + [base * 1.05, base * 0.7, r_edge]
