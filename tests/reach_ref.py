"""The contract of the cost-to-reach field (pwpp_reach_grid, include/pwpp.h) restated as a different algorithm from any kernel: a
binary-heap Dijkstra per frame in Python integers, and the `from` rule applied to its result.  No GPU, no relaxation sweeps."""
import heapq

import numpy as np

NONE = 0x7FFFFFFF
DIST_BEYOND = 0x7FFFFFFF
# the neighbours in the order of their index jy * nx + jx
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def params(base=1, lethal=100, unknown=-1, clearance2=0, max_reach=0):
    return dict(base=base, lethal=lethal, unknown=unknown, clearance2=clearance2, max_reach=max_reach)


def terms(cost, source, p, dist2=None):
    """t of every cell of one (ny, nx) frame as a list of rows of Python ints: 0 impassable, else base + cost."""
    ny, nx = cost.shape
    t = [[0] * nx for _ in range(ny)]
    for y in range(ny):
        for x in range(nx):
            c = int(cost[y, x])
            if c < 0:
                c = p["unknown"]
            ok = 0 <= c < p["lethal"]
            if dist2 is not None and not int(dist2[y, x]) > p["clearance2"]:
                ok = False
            if ok:
                t[y][x] = p["base"] + c
    sx, sy = source
    if t[sy][sx] == 0:
        t[sy][sx] = p["base"]
    return t


def steps_into(t, x, y, nx, ny):
    """(jx, jy, step) for every neighbour with a step to (x, y), in index order."""
    out = []
    if t[y][x] == 0:
        return out
    for dx, dy in NEIGHBOURS:
        jx, jy = x + dx, y + dy
        if not (0 <= jx < nx and 0 <= jy < ny) or t[jy][jx] == 0:
            continue
        if dx != 0 and dy != 0:
            if t[y][jx] == 0 or t[jy][x] == 0:  # the two cells that share an edge with both
                continue
            out.append((jx, jy, 7 * (t[y][x] + t[jy][jx])))
        else:
            out.append((jx, jy, 5 * (t[y][x] + t[jy][jx])))
    return out


def reach_frame(cost, source, p, dist2=None):
    """(reach, from) of one (ny, nx) int8 frame, int32 arrays."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    sx, sy = int(source[0]), int(source[1])
    t = terms(cost, (sx, sy), p, dist2)
    d = {(sx, sy): 0}
    done = set()
    heap = [(0, sy, sx)]
    while heap:
        v, y, x = heapq.heappop(heap)
        if (x, y) in done:
            continue
        done.add((x, y))
        for jx, jy, s in steps_into(t, x, y, nx, ny):  # (steps are symmetric)
            if (jx, jy) not in done and v + s < d.get((jx, jy), 1 << 62):
                d[(jx, jy)] = v + s
                heapq.heappush(heap, (v + s, jy, jx))
    limit = p["max_reach"]
    reach = np.full((ny, nx), NONE, np.int64)
    for (x, y), v in d.items():
        if limit == 0 or v <= limit:
            reach[y, x] = v
    frm = np.full((ny, nx), -1, np.int64)
    for y in range(ny):
        for x in range(nx):
            if reach[y, x] == NONE:
                continue
            if (x, y) == (sx, sy):
                frm[y, x] = y * nx + x
                continue
            for jx, jy, s in steps_into(t, x, y, nx, ny):
                if reach[jy, jx] != NONE and reach[jy, jx] + s == reach[y, x]:
                    frm[y, x] = jy * nx + jx
                    break
            assert frm[y, x] >= 0, "a reached cell without a predecessor"
    assert reach.max() <= NONE
    return reach.astype(np.int32), frm.astype(np.int32)


def reach(cost, source, p, dist2=None):
    """(reach, from) of (frames, ny, nx) or (ny, nx) cost images; source: (sx, sy) or (frames, 2)."""
    cost = np.asarray(cost, np.int8)
    c3 = cost.reshape((1,) + cost.shape) if cost.ndim == 2 else cost
    d3 = None if dist2 is None else np.asarray(dist2, np.int32).reshape(c3.shape)
    src = np.asarray(source, np.int64).reshape(-1, 2)
    out = [reach_frame(c3[f], src[f if len(src) > 1 else 0], p, None if d3 is None else d3[f]) for f in range(c3.shape[0])]
    return np.stack([o[0] for o in out]).reshape(cost.shape), np.stack([o[1] for o in out]).reshape(cost.shape)


def range_ok(base, nx, ny):
    return 14 * (base + 100) * (nx * ny - 1) <= 2 ** 31 - 2


# ---- images the tests share ------------------------------------------------------------------------------------------------------
def random_cost(frames, ny, nx, seed, lethal=0.2, unknown=0.1):
    """int8 costs 0 .. 100 with a share of lethal (100 .. 127) and unknown (-128 .. -1) cells."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 100, (frames, ny, nx)).astype(np.int8)
    u = rng.random((frames, ny, nx))
    c[u < lethal] = rng.integers(100, 128, (frames, ny, nx)).astype(np.int8)[u < lethal]
    c[u > 1.0 - unknown] = rng.integers(-128, 0, (frames, ny, nx)).astype(np.int8)[u > 1.0 - unknown]
    return c


def serpentine(ny, nx, cost=0, wall=100):
    """A corridor one cell wide that runs every other row from end to end; the source belongs at (0, 0)."""
    c = np.full((ny, nx), wall, np.int8)
    c[0::2, :] = cost
    for k, y in enumerate(range(1, ny, 2)):
        c[y, nx - 1 if k % 2 == 0 else 0] = cost
    return c


def spiral(n, cost=0, wall=100):
    """A corridor one cell wide that winds from (0, 0) inwards, walls one cell wide."""
    c = np.full((n, n), wall, np.int8)
    x, y, dx, dy = 0, 0, 1, 0
    c[0, 0] = cost
    seen = {(0, 0)}
    while True:
        moved = False
        for _ in range(2):
            jx, jy = x + dx, y + dy
            kx, ky = jx + dx, jy + dy
            free = 0 <= jx < n and 0 <= jy < n and (jx, jy) not in seen
            # (stop a cell short of a stretch already laid, so that a wall stays between the turns)
            ahead = not (0 <= kx < n and 0 <= ky < n) or (kx, ky) not in seen
            if free and ahead:
                x, y = jx, jy
                c[y, x] = cost
                seen.add((x, y))
                moved = True
                break
            dx, dy = -dy, dx  # turn
        if not moved:
            return c
