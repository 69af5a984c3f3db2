"""Referees and plumbing of the radius-graph tests (tests/test_gpu_graph_edges.py, tests/test_gpu_screening_wide.py,
tests/test_gpu_parity.py and the child processes of the other summation orders): the pair set, one Boruvka round and
the forest contract from the probe's canonical d2 matrix, integer-lattice data whose d2 are exact in every summation
order, and nothing computed on the GPU.  Importing this module needs neither a GPU nor torch."""
import math

import numpy as np

F32 = np.float32
ALL_ONES = np.iinfo(np.uint64).max
NAN, INF = float("nan"), float("inf")


# ---- the radius graph by brute force ------------------------------------------------------------------------------------
def pairs_of(d2, r2):
    """[n_pairs, 2] int64, i < j, sorted: every pair of the d2 matrix with d2 < r2 (strict; none for a NaN r2)"""
    with np.errstate(invalid="ignore"):
        ii, jj = np.nonzero(np.triu(d2 < np.float32(r2), k=1))
    return np.stack([ii, jj], axis=1).astype(np.int64)


def brute_pairs(probe, c, r2):
    """[n_pairs, 2] int64, i < j, sorted: every pair with canonical d2 < r2 (the reference's loop, d2(i,j) = d2(j,i))"""
    return pairs_of(probe.pairwise_d2(c), r2)


def keys(pairs, n):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.minimum(p[:, 0], p[:, 1]) * n + np.maximum(p[:, 0], p[:, 1])


def degrees(pairs, n):
    deg = np.ones(n, dtype=np.int64)
    np.add.at(deg, pairs[:, 0], 1)
    np.add.at(deg, pairs[:, 1], 1)
    return deg


def min_edge_brute(pairs, comp, rank, n):
    """d_best of one round: per component id the smallest (max rank << 32 | min rank) over the pairs that leave it"""
    want = np.full(n, ALL_ONES, dtype=np.uint64)
    a, b = pairs[:, 0], pairs[:, 1]
    cross = comp[a] != comp[b]
    a, b = a[cross], b[cross]
    hi = np.maximum(rank[a], rank[b]).astype(np.uint64)
    lo = np.minimum(rank[a], rank[b]).astype(np.uint64)
    key = (hi << np.uint64(32)) | lo
    np.minimum.at(want, comp[a], key)
    np.minimum.at(want, comp[b], key)
    return want


def components(n, pairs):
    """per frame the smallest frame id of its connected component"""
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)])


def raw_pairs(dens, ct, r2, capacity, rows=None):
    """one dc_hip_radius_pairs_dev call with a buffer of `rows` pairs (default: capacity) prefilled with -1, of which the
    library is told `capacity` -> (count, pairs int32 numpy [rows, 2] or None, pops)"""
    import torch
    from clustering_amd import capi
    n, d = ct.shape
    rows = capacity if rows is None else rows
    assert rows >= capacity
    pops = torch.zeros(n, dtype=torch.int32, device=ct.device)
    count = torch.zeros(1, dtype=torch.int64, device=ct.device)
    pairs = torch.full((rows, 2), -1, dtype=torch.int32, device=ct.device) if rows else None
    ws, ws_bytes = dens._workspace(ct.device).get(n, d, 1)
    with torch.cuda.device(ct.device):
        rc = capi.lib.dc_hip_radius_pairs_dev(dens._dev(ct), n, d, float(r2), dens._dev(pops),
                                              dens._dev(pairs) if pairs is not None else None, capacity,
                                              dens._dev(count), ws, ws_bytes, dens._stream_ptr())
    capi.check(rc, "dc_hip_radius_pairs_dev")
    torch.cuda.synchronize()
    return int(count.item()), (pairs.cpu().numpy() if pairs is not None else None), pops.cpu().numpy()


# ---- ranks and component labels -----------------------------------------------------------------------------------------
RANKS = ("identity", "reversed", "bit-reversed", "random")


def rank_of(kind, n, seed=0):
    """a permutation of 0..n-1 as uint32: the rank of every frame"""
    i = np.arange(n, dtype=np.int64)
    if kind == "identity":
        r = i
    elif kind == "reversed":
        r = n - 1 - i
    elif kind == "bit-reversed":   # (the order of the bit-reversed frame ids: a permutation for every n)
        bits = max(1, int(n - 1).bit_length())
        rev = np.zeros(n, dtype=np.int64)
        for b in range(bits):
            rev |= ((i >> b) & 1) << (bits - 1 - b)
        r = np.empty(n, dtype=np.int64)
        r[np.argsort(rev, kind="stable")] = i
    else:
        r = np.random.default_rng(1000 + n + seed).permutation(n)
    assert np.array_equal(np.sort(r), i)
    return r.astype(np.uint32)


def labels(kind, n, seed=0):
    """component ids per frame (any frame id < n_rows names a component, dc_density.h): "own" every frame its own,
    "one" a single component named by its LAST frame, "any" ~n/6 random components each named by a member that is not
    its smallest"""
    if kind == "own":
        return np.arange(n, dtype=np.uint32)
    if kind == "one":
        return np.full(n, n - 1, dtype=np.uint32)
    rng = np.random.default_rng(2000 + n + seed)
    lab = rng.integers(0, max(1, n // 6), n)
    comp = np.empty(n, dtype=np.uint32)
    for v in np.unique(lab):
        members = np.flatnonzero(lab == v)
        comp[members] = members[-1] if len(members) < 3 else members[1]
    return comp


# ---- lattice data -------------------------------------------------------------------------------------------------------
# integer coordinates in a small range: every partial sum of a d2 is an integer below 2^24, so the sse2, avx and fma
# orders give the same d2 and a radius can be set EQUAL to one.  Exact powers of two and integer shifts keep that.
TRANSFORMS = (("plain", 1.0, 0.0), ("scaled 2^-40", 2.0 ** -40, 0.0), ("scaled 2^20", 2.0 ** 20, 0.0),
              ("shifted 1024", 1.0, 1024.0))


def transformed(c, r2, scale, shift):
    """(c + shift) * scale, and r2 * scale^2"""
    out = ((c.astype(np.float64) + shift) * scale).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), (c.astype(np.float64) + shift) * scale)   # (exact)
    return out, F32(np.float64(F32(r2)) * scale * scale)


def lattice(n, D, seed):
    """n rows with integer coordinates in -1..4: a quarter of them random points of {0..3}^D, the others a step of -1 / 0
    / +1 in a few columns away from one of those (so that small d2 values 0, 1, 2, ... are well populated at every D), in
    shuffled order"""
    rng = np.random.default_rng(seed)
    m = max(1, n // 4)
    base = rng.integers(0, 4, (m, D))
    rows = base[rng.integers(0, m, n)]
    step = rng.choice([-1, 0, 1], size=(n, D), p=[0.5 / (D + 1), 1.0 - 1.0 / (D + 1), 0.5 / (D + 1)])
    return (rows + step).astype(np.float32)


def clustered_lattice(n, D, seed, k=5):
    """k lattice clusters 64 apart along column 0 (far beyond every finite radius used): the spatial order of the sweep
    splits into components, each padded to whole query groups"""
    rng = np.random.default_rng(seed)
    c = lattice(n, D, seed)
    c[:, 0] += 64.0 * rng.integers(0, k, n)
    return c.astype(np.float32)


def tie_radii(d2, level):
    """the squared radii of a tie case at the lattice d2 value `level`: (the float below, level itself, the float above).
    A condition of the case, checked here on the CPU: there are pairs with d2 == r2 for r2 = level (they must stay
    outside) and pairs with d2 == nextafter(r2, 0) for r2 = the float above (they must be inside)."""
    T = F32(level)
    below, above = np.nextafter(T, F32(0.0)), np.nextafter(T, F32(np.inf))
    off = ~np.eye(len(d2), dtype=bool)
    assert T > 0 and (d2[off] == T).any(), f"broken tie case: no pair with d2 == r2 == {T}"
    assert (d2[off] == np.nextafter(above, F32(0.0))).any(), f"broken tie case: no pair one float below r2 == {above}"
    assert (d2[off] < T).any(), f"broken tie case: no pair below {T}"
    return float(below), float(T), float(above)


def level_of(d2, k):
    """the k-th smallest positive value in the d2 matrix"""
    lv = np.unique(d2[d2 > 0])
    return F32(lv[min(k, len(lv) - 1)])


def chain(n):
    """x_i = i in one column: consecutive frames are 1 apart (d2 = 1), all others >= 4"""
    return np.arange(n, dtype=np.float32).reshape(n, 1)


def star(D):
    """a hub at the origin and 2 D leaves at +-2 on every axis -> (coords, r2 = 8, hub id): hub - leaf d2 = 4, leaf - leaf
    d2 = 8 (exactly r2: outside) or 16; frame order shuffled"""
    assert D >= 2
    c = np.zeros((2 * D + 1, D), dtype=np.float32)
    for a in range(D):
        c[1 + 2 * a, a] = 2.0
        c[2 + 2 * a, a] = -2.0
    order = np.random.default_rng(D).permutation(len(c))
    return c[order], 8.0, int(np.flatnonzero(order == 0)[0])


def bridge(D, seed=0):
    """two cliques joined by exactly one pair below r2 = 100 and one pair AT r2 (a decoy that must not link them)
    -> (coords, r2, side [n] 0 / 1, (p, q) the bridge, (d, q) the decoy).  Columns 0 / 1: clique A = 40 frames on
    {0,1}^2 plus p = (9, 0) and d = (2, 0); clique B = 50 frames on {20,21} x {0,1} plus q = (12, 0).  d2(p, q) = 9,
    d2(d, q) = 100, every other A - B pair >= 121, every pair within a clique <= 82.  Frame order shuffled."""
    assert D >= 2
    rng = np.random.default_rng(seed + D)
    xy = np.concatenate([rng.integers(0, 2, (40, 2)), [[9, 0]], [[2, 0]],
                         rng.integers(0, 2, (50, 2)) + [20, 0], [[12, 0]]])
    side = np.concatenate([np.zeros(42, dtype=np.int64), np.ones(51, dtype=np.int64)])
    c = np.zeros((len(xy), D), dtype=np.float32)
    c[:, :2] = xy
    order = rng.permutation(len(c))
    at = {int(f): k for k, f in enumerate(order)}    # original row -> frame id
    return c[order], 100.0, side[order], (at[40], at[92]), (at[41], at[92])


def with_isolated(c, k=7):
    """k more frames far from everything and from each other (multiples of 100 on column 0 past the data), mixed in"""
    D = c.shape[1]
    far = np.zeros((k, D), dtype=np.float32)
    far[:, 0] = float(np.ceil(c[:, 0].max() / 100.0 + 1.0)) * 100.0 + 100.0 * np.arange(k)
    assert far.max() <= 4000.0   # (d2 stay integers below 2^24)
    out = np.concatenate([c, far])
    return out[np.random.default_rng(len(out)).permutation(len(out))]


# ---- the forest contract ------------------------------------------------------------------------------------------------
def check_forest(n, graph_pairs, rank, edges, rounds=None):
    """dc_density.h on dc_hip_radius_forest, at EVERY threshold t: the forest's pairs with max(rank) < t connect exactly
    what the graph's pairs with max(rank) < t connect.  One walk over t with a union-find: the forest pairs of weight t
    join two different sets each (no cycle), after which every graph pair of weight t is connected.  Forest pairs are
    graph pairs, so neither side ever connects more than the other.  Also n_edges = n - #components and, for n >= 2,
    1 <= rounds <= ceil(log2 n) + 1 (every round with a merge at least halves the components that still have a partner
    -- dc_session.hip -- and one last round finds none)."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    graph_pairs = np.asarray(graph_pairs, dtype=np.int64).reshape(-1, 2)
    rank = np.asarray(rank, dtype=np.int64)
    assert ((edges >= 0) & (edges < n)).all(), "a frame id beyond n_rows"
    assert (edges[:, 0] != edges[:, 1]).all(), "a pair of a frame with itself"
    ek, gk = keys(edges, n), keys(graph_pairs, n)
    assert len(np.unique(ek)) == len(ek), "a forest pair listed twice"
    assert np.isin(ek, gk).all(), "a forest pair that is not a pair of the graph"
    w_f = np.maximum(rank[edges[:, 0]], rank[edges[:, 1]]) if len(edges) else np.zeros(0, dtype=np.int64)
    w_g = np.maximum(rank[graph_pairs[:, 0]], rank[graph_pairs[:, 1]]) if len(graph_pairs) else np.zeros(0, dtype=np.int64)
    of, og = np.argsort(w_f, kind="stable"), np.argsort(w_g, kind="stable")
    fa, fb, fw = edges[of, 0].tolist(), edges[of, 1].tolist(), w_f[of].tolist()
    ga, gb, gw = graph_pairs[og, 0].tolist(), graph_pairs[og, 1].tolist(), w_g[og].tolist()
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    i = j = 0
    while i < len(fw) or j < len(gw):
        t = min(fw[i] if i < len(fw) else n, gw[j] if j < len(gw) else n)
        while i < len(fw) and fw[i] == t:
            ra, rb = find(fa[i]), find(fb[i])
            assert ra != rb, f"the forest closes a cycle at weight {t}"
            parent[ra] = rb
            i += 1
        while j < len(gw) and gw[j] == t:
            assert find(ga[j]) == find(gb[j]), \
                f"graph pair ({ga[j]}, {gb[j]}) of weight {t} is not connected by the forest's pairs up to {t}"
            j += 1
    n_comp = len({find(x) for x in range(n)})
    assert len(edges) == n - n_comp, "not a spanning forest"
    if rounds is not None and n >= 2:
        assert 1 <= rounds <= math.ceil(math.log2(n)) + 1, f"{rounds} rounds for {n} rows"
    return n_comp
