"""The obstacle clusters (pwpp_label_grid) restated by the rules of include/pwpp.h: a plain flood fill over the occupied cells of
a count image -- label image, cluster table, number of clusters -- a second, independent restatement (iterated minimum
propagation) to check the first against, and the pattern set the test files run: the small shapes, and the large ones at which a
frame has more chunks than one round of the rank scan takes.  Shared by tests/test_obstacle_clusters_cpu.py,
tests/test_gpu_obstacle_clusters.py and tests/test_gpu_obstacle_clusters_large.py."""
from collections import deque

import numpy as np

from obstacle_grid_ref import F32, height_keys, heights_of_keys

CLUSTER_DTYPE = np.dtype([("first_cell", "<i4"), ("cells", "<i4"), ("points", "<i4"), ("ix_min", "<i4"), ("ix_max", "<i4"),
                          ("iy_min", "<i4"), ("iy_max", "<i4"), ("top", "<f4"), ("sum_ix", "<i8"), ("sum_iy", "<i8")])
assert CLUSTER_DTYPE.itemsize == 48

TILE_X, TILE_Y = 64, 16  # the tile of the library's tile pass: the patterns aim at its edges
SHAPES = [(1, 1), (7, 5), (64, 16), (65, 17), (129, 33), (257, 3), (3, 257)]  # (nx, ny)
PATTERNS = ["empty", "full", "checker", "diagonals", "comb", "spiral", "serpentine", "random0.1", "random0.3", "random0.59", "corner"]

# The large shapes, kept apart from SHAPES (the distance tests import SHAPES).  The ranks come from roots counted per CHUNK of
# PWPP_CL_CHUNK consecutive cells, and one workgroup scans a frame's chunk counts SCAN_BLOCK (kClBlock) at a time with the total
# carried between rounds: a second round needs more than CHUNK * SCAN_BLOCK = 65 536 cells in a frame.
CHUNK = 256       # PWPP_CL_CHUNK of csrc/pwpp_unionfind.h
SCAN_BLOCK = 256  # kClBlock of csrc/pwpp_clusters.hip: chunk counts per round of k_cl_scan
LARGE_SHAPES = [(256, 256), (257, 256), (1030, 132)]
# (nx, ny): cells, chunks, chunks of every scan round, tiles (x, y)
LARGE_PLAN = {(256, 256): (65536, 256, [256], (4, 16)),          # the cost tool's shape: one round, full
              (257, 256): (65792, 257, [256, 1], (5, 16)),         # the last tile column is one cell wide
              (1030, 132): (135960, 532, [256, 256, 20], (17, 9))}  # the last chunk has 24 cells; nx % 64 != 0, ny % 16 != 0
LARGE_PATTERNS = ["random0.1", "random0.3", "random0.59", "checker", "diagonals", "comb", "spiral", "serpentine", "full"]
LARGE_CASES = [(name, 1, c) for name in LARGE_PATTERNS for c in (4, 8)] + [("random0.3", 2, 4), ("random0.3", 2, 8)]  # (name, min_count, connectivity)


def chunk_plan(nx, ny):
    """(cells, chunks, chunks of every scan round, tiles (x, y)) of an nx x ny frame, from CHUNK, SCAN_BLOCK and the tile."""
    cells = nx * ny
    chunks = -(-cells // CHUNK)
    rounds = [min(SCAN_BLOCK, chunks - b) for b in range(0, chunks, SCAN_BLOCK)]
    return cells, chunks, rounds, (-(-nx // TILE_X), -(-ny // TILE_Y))


def roots_beyond(table, chunk):
    """The number of clusters whose first cell lies in chunk `chunk` or a later one: their ranks need the scan that far."""
    return int((table["first_cell"] // CHUNK >= chunk).sum())


def by_construction(name, conn, count, min_count=1):
    """(label, n) of a structured pattern, stated without any search: one cluster on the occupied cells, or, for the checkerboard
    with edge neighbours, every occupied cell a cluster of its own, numbered in row-major order.  None: no such statement."""
    occ = np.asarray(count) >= min_count
    if name in ("full", "comb", "spiral", "serpentine") or (name == "checker" and conn == 8):
        return np.where(occ, 0, -1).astype(np.int32), 1
    if name == "checker" and conn == 4:
        rank = (np.cumsum(occ.reshape(-1)) - 1).reshape(occ.shape)
        return np.where(occ, rank, -1).astype(np.int32), int(occ.sum())
    return None


def neighbours(connectivity):
    assert connectivity in (4, 8)
    edge = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    return edge if connectivity == 4 else edge + [(-1, -1), (1, -1), (-1, 1), (1, 1)]


def table_of(label, n, count, top):
    """The table of one frame from its finished label image: every field by its definition."""
    ny, nx = label.shape
    t = np.zeros(n, CLUSTER_DTYPE)
    iy, ix = np.nonzero(label >= 0)
    r = label[iy, ix]
    c = count[iy, ix].astype(np.int64)
    first = np.full(n, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, r, iy * nx + ix)
    t["first_cell"] = first
    t["cells"] = np.bincount(r, minlength=n)
    t["points"] = np.bincount(r, weights=c, minlength=n).astype(np.int64)
    for name, v, op, start in (("ix_min", ix, np.minimum, nx), ("ix_max", ix, np.maximum, -1), ("iy_min", iy, np.minimum, ny), ("iy_max", iy, np.maximum, -1)):
        a = np.full(n, start, np.int64)
        op.at(a, r, v)
        t[name] = a
    keys = np.zeros(n, np.uint32)
    if top is not None:
        np.maximum.at(keys, r, height_keys(top[iy, ix]))
    t["top"] = heights_of_keys(keys)
    sx, sy = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(sx, r, c * ix)
    np.add.at(sy, r, c * iy)
    t["sum_ix"], t["sum_iy"] = sx, sy
    return t


def flood_fill(count, top=None, min_count=1, connectivity=8):
    """(label (ny, nx) int32, table (n,) CLUSTER_DTYPE, n) of ONE frame.  Seeds are taken in row-major order, so a cluster's
    number is its rank in ascending first_cell."""
    count = np.asarray(count, np.int32)
    ny, nx = count.shape
    occ = count >= min_count
    label = np.full((ny, nx), -1, np.int32)
    nb = neighbours(connectivity)
    n = 0
    for sy, sx in zip(*np.nonzero(occ)):  # (np.nonzero is row-major)
        if label[sy, sx] >= 0:
            continue
        label[sy, sx] = n
        todo = deque([(int(sy), int(sx))])
        while todo:
            y, x = todo.popleft()
            for dx, dy in nb:
                qx, qy = x + dx, y + dy
                if 0 <= qx < nx and 0 <= qy < ny and occ[qy, qx] and label[qy, qx] < 0:
                    label[qy, qx] = n
                    todo.append((qy, qx))
        n += 1
    return label, table_of(label, n, count, None if top is None else np.asarray(top, F32)), n


def min_propagation(count, min_count=1, connectivity=8):
    """The second restatement: every occupied cell starts with its own index and takes the minimum over its occupied neighbours
    until nothing changes; the ranks are the positions of the surviving values in sorted order.  Returns (label, n)."""
    count = np.asarray(count, np.int32)
    ny, nx = count.shape
    occ = count >= min_count
    big = nx * ny
    v = np.where(occ, np.arange(big).reshape(ny, nx), big)
    while True:
        p = np.pad(v, 1, constant_values=big)
        m = v.copy()
        for dx, dy in neighbours(connectivity):
            m = np.minimum(m, p[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx])
        m = np.where(occ, m, big)
        if np.array_equal(m, v):
            break
        v = m
    roots = np.unique(v[occ])
    label = np.full((ny, nx), -1, np.int32)
    label[occ] = np.searchsorted(roots, v[occ])
    return label, len(roots)


def label_frames(count, top=None, min_count=1, connectivity=8, max_clusters=0):
    """What pwpp_label_grid returns for a (frames, ny, nx) image: (label, [table of every frame, cut to max_clusters rows], n)."""
    count = np.asarray(count, np.int32)
    labels, tables, ns = [], [], []
    for f in range(count.shape[0]):
        lab, tab, n = flood_fill(count[f], None if top is None else top[f], min_count, connectivity)
        labels.append(lab)
        tables.append(tab[:max_clusters])
        ns.append(n)
    return np.stack(labels), tables, np.asarray(ns, np.int32)


def same_tables(got, n, want):
    """The first min(n, max_clusters) rows of a returned (max_clusters,) table against the restatement's, bit for bit."""
    k = min(int(n), len(got))
    return len(want) == k and np.ascontiguousarray(got[:k]).tobytes() == np.ascontiguousarray(want).tobytes()


def occupancy(name, nx, ny, rng):
    """The boolean (ny, nx) pattern `name`."""
    y, x = np.mgrid[0:ny, 0:nx]
    if name == "empty":
        return np.zeros((ny, nx), bool)
    if name == "full":
        return np.ones((ny, nx), bool)
    if name == "checker":  # connectivity 4: all singletons; 8: one cluster
        return (x + y) % 2 == 0
    if name == "diagonals":  # both directions, repeated along the longer side
        m = max(min(nx, ny), 2)
        return (x % m == y % m) | ((nx - 1 - x) % m == y % m)
    if name == "comb":  # teeth in every other column that join only in the last row: the classic late equivalence
        return (x % 2 == 0) | (y == ny - 1)
    if name == "serpentine":  # every other row, joined at alternating ends: it crosses every tile edge
        return (y % 2 == 0) | (x == np.where((y // 2) % 2 == 0, nx - 1, 0))
    if name == "corner":  # two blocks that touch only at a tile corner (connectivity 4: two clusters, 8: one)
        a = (x < TILE_X) & (x >= TILE_X - 3) & (y < TILE_Y) & (y >= TILE_Y - 3)
        b = (x >= TILE_X) & (x < TILE_X + 3) & (y >= TILE_Y) & (y < TILE_Y + 3)
        return a | b
    if name == "spiral":  # one cell wide from the rim to the centre, a free lane between the turns: the longest chase
        occ = np.zeros((ny, nx), bool)
        cx, cy, d, stuck = 0, 0, 0, 0
        occ[0, 0] = True
        while stuck < 2:  # walk on while the next cell is inside and free and the one behind it is free; turn right otherwise
            dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[d]
            qx, qy, ax, ay = cx + dx, cy + dy, cx + 2 * dx, cy + 2 * dy
            # (never back onto the path: on a square of even side the walk would otherwise circle in the centre for ever; the
            # pattern of every shape at which it ended without this is unchanged)
            if 0 <= qx < nx and 0 <= qy < ny and not occ[qy, qx] and not (0 <= ax < nx and 0 <= ay < ny and occ[ay, ax]):
                cx, cy, stuck = qx, qy, 0
                occ[cy, cx] = True
            else:
                d, stuck = (d + 1) % 4, stuck + 1
        return occ
    if name.startswith("random"):  # 0.59: near the percolation threshold of the square lattice, large ragged clusters
        return rng.random((ny, nx)) < float(name[6:])
    raise ValueError(name)


def pattern(name, nx, ny, min_count, seed=0):
    """(count int32, top float32) of the pattern: counts from 0..3, the pattern's cells min_count..3 and the others below
    min_count; top a height where count > 0 and the quiet NaN elsewhere, as pwpp_rasterize_obstacles writes it."""
    rng = np.random.default_rng([seed, nx, ny, min_count, PATTERNS.index(name)])
    occ = occupancy(name, nx, ny, rng)
    count = np.where(occ, rng.integers(min_count, 4, (ny, nx)), rng.integers(0, min_count, (ny, nx))).astype(np.int32)
    top = np.where(count > 0, rng.uniform(-1.0, 3.0, (ny, nx)), np.nan).astype(F32)
    return count, top
