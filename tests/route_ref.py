"""The contract of the routes on the reach field (pwpp_route_grid, pwpp_plan_grid, include/pwpp.h) restated in plain Python on top of
tests/reach_ref.py: the chain walk, the row, THE LINE written out again from its closed form, the greedy waypoints.  No GPU, no window,
no ballot.

`certify` decides whether a given route IS the route of a start without walking `from` or searching: every hop must be a step of the
reach contract onto a strictly smaller reach that the hop accounts for exactly (and, with tie_break, the first such neighbour in index
order), the sums must be those of the cells, every shortcut's rasterised line a legal step path within line_cost, and no candidate
beyond a chosen waypoint within `look` may have such a line."""
import numpy as np

import reach_ref as rr

OK, NONE, BROKEN = 0, 1, 2
BEYOND = rr.DIST_BEYOND
ROW = np.dtype([(n, "<i4") for n in ("status", "cells", "cost", "edge_steps", "corner_steps", "max_term", "min_dist2", "waypoints")])


def route_params(max_cells=0, max_waypoints=0, look=1, line_cost=0):
    return dict(max_cells=max_cells, max_waypoints=max_waypoints, look=look, line_cost=line_cost)


def term(t, x, y):
    """t of a cell anywhere: 0 outside the image; t: the rows of reach_ref.terms."""
    return t[y][x] if 0 <= y < len(t) and 0 <= x < len(t[0]) else 0


def hop(t, nx, ny, c, n):
    """(step, corner) of the hop c -> n, n any integer, or None where it is no step of the contract."""
    if not 0 <= n < nx * ny:
        return None
    cx, cy, ex, ey = c % nx, c // nx, n % nx, n // nx
    dx, dy = ex - cx, ey - cy
    if max(abs(dx), abs(dy)) != 1:
        return None
    if term(t, cx, cy) == 0 or term(t, ex, ey) == 0:
        return None
    corner = dx != 0 and dy != 0
    if corner and (term(t, ex, cy) == 0 or term(t, cx, ey) == 0):
        return None
    return (7 if corner else 5) * (term(t, cx, cy) + term(t, ex, ey)), corner


def line(ax, ay, bx, by):
    """THE LINE of csrc/pwpp_visibility.h from a to b by its closed form: P_0 .. P_n."""
    dx, dy = bx - ax, by - ay
    n = max(abs(dx), abs(dy))
    sgn = lambda v: (v > 0) - (v < 0)
    if n == 0:
        return [(ax, ay)]
    return [(ax + sgn(dx) * ((2 * k * abs(dx) + n) // (2 * n)), ay + sgn(dy) * ((2 * k * abs(dy) + n) // (2 * n))) for k in range(n + 1)]


def line_clear(t, a, b, limit):
    """Whether the line from the cell a = (x, y) to b is clear: 0 < t(P_k) <= limit for k >= 1, both squeezed cells passable."""
    pts = line(a[0], a[1], b[0], b[1])
    for (px, py), (x, y) in zip(pts, pts[1:]):
        if x != px and y != py and (term(t, px, y) == 0 or term(t, x, py) == 0):
            return False
        if not 0 < term(t, x, y) <= limit:
            return False
    return True


def walk(t, d2, frm, nx, ny, start, source):
    """(row as a dict, cells) of the chain from the cell index `start`; frm: the frame's from, flat; d2: flat or None."""
    row = dict(status=NONE, cells=0, cost=0, edge_steps=0, corner_steps=0, max_term=0, min_dist2=BEYOND, waypoints=0)
    if frm[start] == -1:
        return row, []
    cells = [start]
    c = start
    status = None
    while status is None:
        n = int(frm[c])
        if n == c:
            status = OK if c == source else BROKEN
            break
        h = hop(t, nx, ny, c, n) if len(cells) - 1 < nx * ny - 1 else None
        if h is None:
            status = BROKEN
            break
        row["cost"] += h[0]
        row["corner_steps" if h[1] else "edge_steps"] += 1
        cells.append(n)
        c = n
    row["status"], row["cells"] = status, len(cells)
    row["max_term"] = max(term(t, i % nx, i // nx) for i in cells)
    row["min_dist2"] = BEYOND if d2 is None else min(int(d2[i]) for i in cells)
    return row, cells


def greedy(t, nx, cells, look, limit):
    """The waypoints of a route that arrived, as indices into it."""
    xy = lambda i: (cells[i] % nx, cells[i] // nx)
    w, a, last = [0], 0, len(cells) - 1
    while a < last:
        b = next((b for b in range(min(a + look, last), a + 1, -1) if line_clear(t, xy(a), xy(b), limit)), a + 1)
        w.append(b)
        a = b
    return w


def route_frame(cost, source, p, frm, starts, q, dist2=None):
    """(rows, cells, waypoints) of one (ny, nx) frame: ROW (n,), int32 (n, max_cells), int32 (n, max_waypoints)."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    sx, sy = int(source[0]), int(source[1])
    t = rr.terms(cost, (sx, sy), p, dist2)
    f = np.asarray(frm).reshape(-1)
    d2 = None if dist2 is None else np.asarray(dist2).reshape(-1)
    starts = np.asarray(starts).reshape(-1, 2)
    rows = np.zeros(len(starts), ROW)
    cl = np.full((len(starts), q["max_cells"]), -1, np.int32)
    wp = np.full((len(starts), q["max_waypoints"]), -1, np.int32)
    for k, (x, y) in enumerate(starts):
        row, cells = walk(t, d2, f, nx, ny, int(y) * nx + int(x), sy * nx + sx)
        m = min(len(cells), q["max_cells"])
        cl[k, :m] = cells[:m]
        if row["status"] == OK and q["max_waypoints"] > 0:
            w = [cells[i] for i in greedy(t, nx, cells, q["look"], p["base"] + q["line_cost"])]
            row["waypoints"] = len(w)
            m = min(len(w), q["max_waypoints"])
            wp[k, :m] = w[:m]
        for name in ROW.names:
            rows[k][name] = row[name]
    return rows, cl, wp


def routes(cost, source, p, frm, start, q, dist2=None):
    """(rows (frames, n), cells (frames, n, max_cells), waypoints (frames, n, max_waypoints)) of (frames, ny, nx) cost images; start:
    (n, 2) for every frame or (frames, n, 2)."""
    cost = np.asarray(cost, np.int8)
    c3 = cost.reshape((1,) + cost.shape) if cost.ndim == 2 else cost
    f3 = np.asarray(frm, np.int32).reshape(c3.shape)
    d3 = None if dist2 is None else np.asarray(dist2, np.int32).reshape(c3.shape)
    src = np.asarray(source, np.int64).reshape(-1, 2)
    st = np.asarray(start, np.int64)
    st = st.reshape(1, -1, 2) if st.ndim < 3 else st
    out = [route_frame(c3[f], src[f if len(src) > 1 else 0], p, f3[f], st[f if len(st) > 1 else 0], q, None if d3 is None else d3[f]) for f in range(len(c3))]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def plan(cost, source, p, start, q, dist2=None):
    """reach_ref.reach, then routes on its from."""
    _, frm = rr.reach(cost, source, p, dist2)
    return routes(cost, source, p, frm, start, q, dist2)


def certify(cost, source, p, reach, start, q, row, cells, waypoints, dist2=None, tie_break=True):
    """None where (row, cells, waypoints) -- the whole lists, cell indices -- is the route of the cell `start` = (x, y) on the reach field
    `reach` of the (ny, nx) frame, else a reason.  Walks nothing and searches nothing: it judges the lists it is given."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    sx, sy = int(source[0]), int(source[1])
    t = rr.terms_array(cost, (sx, sy), p, dist2).tolist()
    v = np.asarray(reach).astype(np.int64)
    s = int(start[1]) * nx + int(start[0])
    cells = [int(c) for c in cells]
    if v[start[1], start[0]] == rr.NONE:
        good = row["status"] == NONE and not cells and not len(waypoints) and all(row[n] == 0 for n in ROW.names[1:] if n != "min_dist2") and row["min_dist2"] == BEYOND
        return None if good else "an unreachable start with a route"
    if row["status"] != OK:
        return "status %d for a reachable start" % row["status"]
    if not cells or cells[0] != s or cells[-1] != sy * nx + sx:
        return "the cell list does not run from the start to the source"
    edge = corner = 0
    for c, n in zip(cells, cells[1:]):
        x, y = c % nx, c // nx
        into = rr.steps_into(t, x, y, nx, ny)  # (jx, jy, step), in index order
        attain = [(jy * nx + jx, st) for jx, jy, st in into if v[jy, jx] != rr.NONE and v[jy, jx] + st == v[y, x]]
        if n not in [a[0] for a in attain]:
            return "the hop %d -> %d is no step onto a reach that accounts for it" % (c, n)
        if not v[n // nx, n % nx] < v[y, x]:
            return "the hop %d -> %d does not fall" % (c, n)
        if tie_break and n != attain[0][0]:
            return "the hop %d -> %d: the first neighbour that attains the value is %d" % (c, n, attain[0][0])
        if n % nx != x and n // nx != y:
            corner += 1
        else:
            edge += 1
    tt = [t[c // nx][c % nx] for c in cells]
    want = dict(cells=len(cells), cost=int(v[start[1], start[0]]), edge_steps=edge, corner_steps=corner, max_term=max(tt),
                min_dist2=BEYOND if dist2 is None else int(min(np.asarray(dist2).reshape(-1)[c] for c in cells)))
    for name, value in want.items():
        if row[name] != value:
            return "%s is %d, not %d" % (name, row[name], value)
    if q["max_waypoints"] == 0:
        return None if row["waypoints"] == 0 and not len(waypoints) else "waypoints without a search"
    at = {c: i for i, c in enumerate(cells)}  # (reach falls along the route: no cell twice)
    if any(int(w) not in at for w in waypoints):
        return "a waypoint off the route"
    w = [at[int(c)] for c in waypoints]
    last = len(cells) - 1
    if row["waypoints"] != len(w) or not w or w[0] != 0 or w[-1] != last:
        return "the waypoints do not run from the start to the source"
    limit = p["base"] + q["line_cost"]

    def legal(a, b):  # the rasterised line as a step path within the limit
        pts = line(cells[a] % nx, cells[a] // nx, cells[b] % nx, cells[b] // nx)
        for (px, py), (x, y) in zip(pts, pts[1:]):
            if not any((jx, jy) == (px, py) for jx, jy, _ in rr.steps_into(t, x, y, nx, ny)) or t[y][x] > limit:
                return False
        return True

    for a, b in zip(w, w[1:]):
        if not a < b <= a + q["look"]:
            return "waypoint %d after %d with look %d" % (b, a, q["look"])
        if b > a + 1 and not legal(a, b):
            return "the line from waypoint %d to %d is no legal path within line_cost" % (a, b)
        for far in range(b + 1, min(a + q["look"], last) + 1):
            if legal(a, far):
                return "waypoint %d after %d although the line to %d is clear" % (b, a, far)
    return None


def lists_of(row, cells, waypoints):
    """The stored lists of one route without their -1 tails (the whole lists where the limits were large enough)."""
    return [int(c) for c in cells[:min(int(row["cells"]), len(cells))]], [int(c) for c in waypoints[:min(int(row["waypoints"]), len(waypoints))]]
