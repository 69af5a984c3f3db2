"""Where the pruned self sweeps of 1 - 64 columns may read and write (clustering_amd/bin/test_pruned_ws_model, a host
program: tests/cpp/test_pruned_ws_model.hip).  The library's own launchers and dispatch templates run on the CPU with their
launches recorded instead of started; for every kernel the program states from the kernel's indexing which bytes it touches, and asserts that
they lie inside the workspace of dc_hip_workspace_bytes (or the caller's array), that no range runs into the next region of
the layout, that ranges of one call overlap only where the code declares an alias and in the launch order that makes it
safe, that the padded orders, the reference shares and the segments' deal are consistent, and that the block and the dynamic
LDS of every launch fit what the kernel declares and indexes; a 64-lane model of the pair sink shows reserved == stored.  Over 24 row counts x both ends of every MFMA count's column range x every call kind, and under the
switch settings the GPU tests use (the switches are read by the library itself, from the environment).  DESIGN.md 4.35
records the three seeded faults this fails on."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "clustering_amd", "bin", "test_pruned_ws_model")
SWITCHES = ("DC_POP_SYM", "DC_POP_SHARED", "DC_NN_SHARED", "DC_WAVES_PER_GROUP", "DC_NN_COOP", "DC_NN_RHO", "DC_WAVE_TARGET",
            "DC_SHARE_FLOOR", "DC_POP_COMPONENTS", "DC_POP_CELL_FRAMES", "DC_NN_CELL_FRAMES", "DC_NN_FE_BITS", "DC_SWEEP_DISPATCH",
            "DC_SWEEP_SLOTS")
# the forms of tests/test_gpu_pruned_edges.py and tests/test_gpu_sweep_tickets.py, and the one setting under which the
# regrouped boxes of the neighbour sweep need their last pad box (shared operands: groups of 512 rows; 64 shares)
SETTINGS = {
    "default": {},
    "one-sided": {"DC_POP_SYM": "0"},
    "four waves": {"DC_WAVES_PER_GROUP": "4"},
    "pop and nn shared": {"DC_POP_SHARED": "1", "DC_NN_SHARED": "1"},
    "nn shared floor 8": {"DC_NN_SHARED": "1", "DC_SHARE_FLOOR": "8"},
    "coop floor 8": {"DC_NN_COOP": "1", "DC_SHARE_FLOOR": "8"},
    "no coop floor 16": {"DC_NN_COOP": "0", "DC_SHARE_FLOOR": "16"},
    "floor 16 target 4000": {"DC_SHARE_FLOOR": "16", "DC_WAVE_TARGET": "4000"},
    "static, no components": {"DC_SWEEP_DISPATCH": "static", "DC_POP_COMPONENTS": "0"},
}
CALLS = 187250     # calls of the grid in the program's source: the same under every setting (the launches differ)


@pytest.mark.parametrize("name", list(SETTINGS))
def test_every_index_of_the_pruned_sweeps_stays_in_its_region(name):
    assert os.path.exists(EXE), "build() makes clustering_amd/bin/test_pruned_ws_model"
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(SETTINGS[name])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-3000:] + out.stderr[-2000:]
    launches, calls = (int(x) for x in out.stdout.split()[1:3])
    assert calls == CALLS and launches > 10 * calls, (launches, calls)


def _components(c, r_conn, f32):
    """the host-visible part of fine_mark_kernel / components_kernel (dc_mfma.hip) for coordinates c and a connectivity
    length: coarse grid, occupied sub-cells, boxes of the occupied coarse cells, cells joined where their boxes come
    within r_conn -> (component of every row, number of components as the kernel decides it)"""
    import numpy as np
    k_coarse, k_sub, k_max_comp = 128, 4, 64
    x, y = c[:, 0].astype(f32), (c[:, 1] if c.shape[1] > 1 else np.zeros(len(c))).astype(f32)
    min0, min1 = x.min(), y.min()
    e0, e1 = f32(x.max() - min0), f32(y.max() - min1)
    gc = max(f32(0.5) * f32(r_conn), f32(max(e0, e1) / f32(k_coarse - 1)))
    ncx = min(int(min(f32(e0 / gc), f32(k_coarse))) + 1, k_coarse)
    ncy = min(int(min(f32(e1 / gc), f32(k_coarse))) + 1, k_coarse)
    gf = f32(gc / f32(k_sub))
    fx = np.minimum(np.maximum((x - min0) / gf, 0), ncx * k_sub - 1).astype(np.int64)
    fy = np.minimum(np.maximum((y - min1) / gf, 0), ncy * k_sub - 1).astype(np.int64)
    cell = (fx // k_sub) * ncy + fy // k_sub
    slack = f32(1.0e-3) * gf
    boxes = {}
    for cc in np.unique(cell):
        m = cell == cc
        boxes[int(cc)] = (min0 + fx[m].min() * gf - slack, min0 + (fx[m].max() + 1) * gf + slack,
                          min1 + fy[m].min() * gf - slack, min1 + (fy[m].max() + 1) * gf + slack)
    cells = sorted(boxes)
    root = {cc: cc for cc in cells}

    def find(a):
        while root[a] != a:
            a = root[a]
        return a
    r2c = f32(r_conn) * f32(r_conn) * f32(1.0002)
    for i, a in enumerate(cells):
        for b in cells[i + 1:]:
            ba, bb = boxes[a], boxes[b]
            dx = max(0.0, max(ba[0] - bb[1], bb[0] - ba[1]))
            dy = max(0.0, max(ba[2] - bb[3], bb[2] - ba[3]))
            if dx * dx + dy * dy <= r2c:
                root[max(find(a), find(b))] = min(find(a), find(b))
    roots = sorted({find(cc) for cc in cells})
    if len(cells) > 2048 or len(roots) > k_max_comp or len(roots) <= 1:
        return np.zeros(len(c), dtype=np.int64), 1
    return np.array([roots.index(find(int(cc))) for cc in cell]), len(roots)


def test_replay_of_the_pair_list_case_that_faulted():
    """test_sessions_of_several_devices[n2000-D3-G2-allreduce] (tests/test_gpu_session_edges.py) met an illegal memory access
    in its pair list.  What the host can know of those three calls, replayed from the case's own data: the components under
    both connectivity lengths (count only: r_max / 2; with a buffer: r_max), the padded order order_meta_kernel lays out
    for groups of tq_pop(1) = 6 tiles, the tiles of query_plan and of the layout, and the pair count against the three
    capacities.  Every figure is inside the bounds the model program asserts for any data."""
    import sys
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import sessionref as S
    from graphref import pairs_of
    f32 = np.float32
    n, D, group_rows, k_max_comp, pad_tiles = 2000, 3, 32 * 6, 64, 64 * 512 // 32
    c, _ = S.multi_data((n, D, 2, "allreduce", None))
    d2 = ((c[:, None, :].astype(np.float64) - c[None, :, :]) ** 2).sum(-1).astype(f32)     # integers: exact in every order

    class Ref:
        pass
    ref = Ref()
    ref.d2, ref.n = d2, n
    from prunedref import off_diagonal
    ref.d2x = off_diagonal(d2)
    r2 = S.radii_of(ref)["r2"]["above"]
    assert f32(r2) == np.nextafter(f32(2.0), f32(np.inf))
    count = len(pairs_of(d2, r2))
    assert count == 313542                      # the three calls: capacity 0, 313542 and 156771 (the only one with count > capacity)
    r_max = f32(np.sqrt(f32(r2))) * f32(1.0001)
    T = (n + 31) // 32
    T_r = (n + k_max_comp * (group_rows - 1) + 31) // 32
    assert T_r == 445 and T_r <= T + pad_tiles
    for r_conn, want_comps in ((f32(0.5) * r_max, 36), (r_max, 1)):
        comp, n_comp = _components(c, r_conn, f32)
        assert n_comp == want_comps            # 36 lattice sites of the plane, one component each / all joined
        rows = np.bincount(comp, minlength=k_max_comp)
        padded = ((rows + group_rows - 1) // group_rows) * group_rows
        base = np.concatenate([[0], np.cumsum(padded)])
        assert rows.sum() == n and base[-1] <= 32 * T_r and base[-1] % group_rows == 0
        # every group of 6 tiles holds the rows of one component only; the groups behind the last component are all pad
        assert (padded[rows > 0] >= rows[rows > 0]).all() and base[-1] // group_rows <= -(-T_r // 6)
    # positions fit the 24 bits of a queue entry; a pair buffer of `count` pairs holds 8 * count bytes
    assert 32 * T_r <= 1 << 24
