"""The obstacle hulls (pwpp_hull_obstacles, pwpp_hull_points) restated from include/pwpp.h in Python integers and numpy doubles: the
hull by Andrew's monotone chain -- deliberately another algorithm than the library's march -- the rectangle by trying every edge with
unbounded integers, the six floats through numpy float64 + - * / sqrt (float(int) is the correctly rounded conversion of a big
integer, numpy forms no FMA).  Shared by tests/test_obstacle_hulls_cpu.py and tests/test_gpu_obstacle_hulls.py."""
from fractions import Fraction

import numpy as np

from obstacle_grid_ref import F32, QNAN_BITS, cells_of

F64 = np.float64
FLOATS = ("cx", "cy", "ax", "ay", "length", "width")
HULL_DTYPE = np.dtype([("points", "<i4"), ("n_vertices", "<i4"), ("stored", "<i4"), ("rect_edge", "<i4"), ("area2", "<i8"),
                       ("qx_min", "<i4"), ("qx_max", "<i4"), ("qy_min", "<i4"), ("qy_max", "<i4")] + [(n, "<f4") for n in FLOATS])
assert HULL_DTYPE.itemsize == 64
QMAX = (1 << 20) + 1


def cross(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def hull(points):
    """The strict convex hull of integer pairs: counter-clockwise, from the vertex with the smallest (qy, qx)."""
    pts = sorted(set((int(x), int(y)) for x, y in points))
    if len(pts) <= 1:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    ring = lower[:-1] + upper[:-1]
    k = min(range(len(ring)), key=lambda i: (ring[i][1], ring[i][0]))
    return ring[k:] + ring[:k]


def edge(v, i):
    """(W, H, L2, ex, ey, pmin, pmax, qmin, qmax) of edge i of the vertex list v."""
    n = len(v)
    ex, ey = (1, 0) if n == 1 else (v[(i + 1) % n][0] - v[i][0], v[(i + 1) % n][1] - v[i][1])
    if ex < 0 or (ex == 0 and ey < 0):
        ex, ey = -ex, -ey
    p = [ex * x + ey * y for x, y in v]
    q = [ex * y - ey * x for x, y in v]
    return (max(p) - min(p), max(q) - min(q), ex * ex + ey * ey, ex, ey, min(p), max(p), min(q), max(q))


def rectangle(v):
    """(the chosen edge, its tuple of edge()): the first edge of least W * H / L2."""
    best, at = None, -1
    for i in range(len(v)):
        e = edge(v, i)
        if best is None or e[0] * e[1] * best[2] < best[0] * best[1] * e[2]:
            best, at = e, i
    return at, best


def rect_floats(e, x0, y0):
    W, H, L2, ex, ey, pmin, pmax, qmin, qmax = e
    x0, y0 = F64(x0), F64(y0)
    L = np.sqrt(F64(L2))
    U = (pmin + pmax) * ex - (qmin + qmax) * ey
    V = (pmin + pmax) * ey + (qmin + qmax) * ex
    d = F64(2.0) * F64(L2)
    return (F32(x0 + (F64(float(U)) / d) / F64(1024.0)), F32(y0 + (F64(float(V)) / d) / F64(1024.0)), F32(F64(ex) / L), F32(F64(ey) / L),
            F32((F64(W) / L) / F64(1024.0)), F32((F64(H) / L) / F64(1024.0)))


def hull_row(points, x0, y0, max_vertices):
    """(the row, its full vertex list) of one row's integer pairs, duplicates included."""
    o = np.zeros((), HULL_DTYPE)
    for name in FLOATS:
        o[name] = np.uint32(QNAN_BITS).view(F32)
    o["rect_edge"] = -1
    if len(points) == 0:
        return o, []
    v = hull(points)
    n = len(v)
    o["points"], o["n_vertices"], o["stored"] = len(points), n, min(n, max_vertices)
    o["area2"] = sum(v[i][0] * v[(i + 1) % n][1] - v[(i + 1) % n][0] * v[i][1] for i in range(n))
    o["qx_min"], o["qx_max"] = min(p[0] for p in v), max(p[0] for p in v)
    o["qy_min"], o["qy_max"] = min(p[1] for p in v), max(p[1] for p in v)
    if n <= max_vertices:
        at, e = rectangle(v)
        o["rect_edge"] = at
        for name, f in zip(FLOATS, rect_floats(e, x0, y0)):
            o[name] = f
    return o, v


def quantise(x0, y0, xyz):
    """The (m, 2) int64 pairs of (m, 3) float32 positions."""
    xyz = np.nan_to_num(np.ascontiguousarray(xyz, F32).reshape(-1, 3), nan=0.0)   # (a NaN position is never kept)
    qx = np.rint((xyz[:, 0].astype(F64) - F64(x0)) * F64(1024.0)).astype(np.int64)
    qy = np.rint((xyz[:, 1].astype(F64) - F64(y0)) * F64(1024.0)).astype(np.int64)
    return np.stack([qx, qy], 1)


def hull_rows(x0, y0, cell, nx, ny, xyz, row, max_hulls, max_vertices):
    """What pwpp_hull_points returns: the (max_hulls,) rows and, per row, the full vertex list (compare its first `stored`)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    row = np.ascontiguousarray(row, np.int32).reshape(-1)
    kx, _ = cells_of(xyz[:, 0], F64(x0), cell, nx)
    ky, _ = cells_of(xyz[:, 1], F64(y0), cell, ny)
    keep = kx & ky & ~np.isnan(xyz[:, 2]) & (row >= 0) & (row < max_hulls)
    q = quantise(x0, y0, xyz)
    out, lists = np.zeros(max_hulls, HULL_DTYPE), []
    for r in range(max_hulls):
        o, v = hull_row([tuple(p) for p in q[keep & (row == r)].tolist()], x0, y0, max_vertices)
        out[r] = o
        lists.append(v)
    return out, lists


def same(rows, lists, ref_rows, ref_lists, what=""):
    """Rows byte for byte; of the lists the first `stored` entries of every row (the rest is unspecified).  lists may be None."""
    rows, ref_rows = np.ascontiguousarray(rows).reshape(-1), np.ascontiguousarray(ref_rows).reshape(-1)
    assert rows.dtype == HULL_DTYPE and rows.shape == ref_rows.shape, what
    for r in range(len(rows)):
        assert rows[r].tobytes() == ref_rows[r].tobytes(), "%s row %d:\n%s\n%s" % (what, r, rows[r], ref_rows[r])
    if lists is not None:
        lists = np.asarray(lists).reshape(len(rows), -1, 2)
        for r in range(len(rows)):
            k = int(ref_rows[r]["stored"])
            assert lists[r, :k].tolist() == [list(p) for p in ref_lists[r][:k]], "%s row %d: vertices" % (what, r)


def box_area_not_below(hull_entry, ax, ay, points):
    """The header's invariant in exact rationals: W * H / L2 of the chosen edge <= the area of the rectangle that encloses the
    integer points along the box's float axis (ax, ay)."""
    W, H, L2 = hull_entry[:3]
    ux, uy = Fraction(float(ax)), Fraction(float(ay))
    p = [ux * x + uy * y for x, y in points]
    q = [ux * y - uy * x for x, y in points]
    return Fraction(W * H, L2) <= (max(p) - min(p)) * (max(q) - min(q)) / (ux * ux + uy * uy)
