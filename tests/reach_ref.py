"""The contract of the cost-to-reach field (pwpp_reach_grid, include/pwpp.h) restated as a different algorithm from any kernel: a
binary-heap Dijkstra per frame in Python integers, and the `from` rule applied to its result.  No GPU, no relaxation sweeps.

For frames too large for that Dijkstra (about 50 000 cells): `certify`, which decides in a few numpy passes whether a given field IS the
reach field, by the fixed-point argument of csrc/pwpp_reach.h, and `reach_flat`, a second Dijkstra on flat lists that the tests pin to
the first one where both can run.  `comb` and `chain` make and judge the images of the many-tile tests."""
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


# ---- large frames: one vectorised statement of the rule, a check of a finished field and a faster Dijkstra -------------------------------
def terms_array(cost, source, p, dist2=None):
    """`terms` in numpy: t of every cell of one (ny, nx) frame as int64; source None: no cell is made passable."""
    c = np.asarray(cost).astype(np.int64)
    c = np.where(c < 0, p["unknown"], c)
    ok = (c >= 0) & (c < p["lethal"])
    if dist2 is not None:
        ok &= np.asarray(dist2).astype(np.int64) > p["clearance2"]
    t = np.where(ok, p["base"] + c, 0)
    if source is not None and t[source[1], source[0]] == 0:
        t[source[1], source[0]] = p["base"]
    return t


def shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that lies outside."""
    ny, nx = a.shape
    b = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -dy), ny - max(0, dy), max(0, -dx), nx - max(0, dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return b


_BIG = 1 << 62


def offers(t, v, limit):
    """For every cell the smallest v(n) + step(n, c) over its 8 neighbours (_BIG: none) and the k of the first neighbour in index
    order that offers it (-1); a candidate above `limit` (> 0) is dropped, the corner rule applies.  t, v: int64; v NONE: no value."""
    best = np.full(t.shape, _BIG, np.int64)
    first = np.full(t.shape, -1, np.int64)
    for k, (dx, dy) in enumerate(NEIGHBOURS):
        tn, vn = shifted(t, dx, dy, 0), shifted(v, dx, dy, NONE)
        ok = (t > 0) & (tn > 0) & (vn != NONE)
        if dx != 0 and dy != 0:
            ok &= (shifted(t, dx, 0, 0) > 0) & (shifted(t, 0, dy, 0) > 0)  # the two cells that share an edge with both
        cand = vn + (7 if dx != 0 and dy != 0 else 5) * (t + tn)
        if limit > 0:
            ok &= cand <= limit
        better = ok & (cand < best)  # (strictly: the first in index order stays)
        best = np.where(better, cand, best)
        first = np.where(better, k, first)
    return best, first


def from_of(first, source):
    """The from image of the `first` of offers (-1 stays -1); the source names itself."""
    ny, nx = first.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    ddx, ddy = np.array([n[0] for n in NEIGHBOURS] + [0]), np.array([n[1] for n in NEIGHBOURS] + [0])
    frm = np.where(first >= 0, (yy + ddy[first]) * nx + xx + ddx[first], -1)
    frm[source[1], source[0]] = source[1] * nx + source[0]
    return frm


def certify(cost, source, p, reach, frm, dist2=None):
    """None where (reach, frm) -- frm None: not looked at -- is the reach field of the (ny, nx) frame, else (reason, (x, y)) with the first
    offending cell in index order.  The field is the reach field exactly when the source holds 0, no cell with term 0 holds a value, and
    every other cell holds the minimum over its 8 neighbours of v(n) + step(n, c), candidates above max_reach dropped, or NONE where no
    neighbour offers one: the fixed point gives v <= d along a shortest path; the neighbour that attains a cell's minimum holds a strictly
    smaller value, so the chain of such neighbours ends -- at the one cell the equation is not asked of, the source -- and spells a real
    path of length v, so v >= d; an unreached cell with d <= max_reach has its predecessor, reached by induction, offering it d.  from is
    the first neighbour in index order that attains the minimum, the source's its own index, -1 beside NONE."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    sx, sy = int(source[0]), int(source[1])
    v = np.asarray(reach).astype(np.int64)
    if v.shape != (ny, nx):
        return "reach has the shape %r, not %r" % (v.shape, (ny, nx)), (0, 0)
    t = terms_array(cost, (sx, sy), p, dist2)

    def fail(bad, text):
        y, x = (int(q) for q in np.argwhere(bad)[0])
        return text(x, y), (x, y)

    if v[sy, sx] != 0:
        return "the source holds %d, not 0" % v[sy, sx], (sx, sy)
    bad = (t == 0) & (v != NONE)
    if bad.any():
        return fail(bad, lambda x, y: "the impassable cell (%d, %d) holds %d" % (x, y, v[y, x]))
    best, first = offers(t, v, p["max_reach"])
    want = np.where(best == _BIG, NONE, best)
    want[sy, sx] = 0
    bad = v != want
    if bad.any():
        def text(x, y):
            if want[y, x] == NONE:
                return "cell (%d, %d) holds %d and no neighbour offers a value" % (x, y, v[y, x])
            if v[y, x] == NONE:
                return "cell (%d, %d) holds none and a neighbour offers %d" % (x, y, want[y, x])
            return "cell (%d, %d) holds %d, %s the %d its neighbours offer" % (x, y, v[y, x], "above" if v[y, x] > want[y, x] else "below", want[y, x])
        return fail(bad, text)
    if frm is None:
        return None
    f = np.asarray(frm).astype(np.int64)
    if f.shape != (ny, nx):
        return "from has the shape %r, not %r" % (f.shape, (ny, nx)), (0, 0)
    want_from = from_of(first, (sx, sy))
    bad = f != want_from
    if bad.any():
        return fail(bad, lambda x, y: "from of cell (%d, %d) is %d, the first neighbour that attains its value is %d" % (x, y, f[y, x], want_from[y, x]))
    return None


def reach_flat(cost, source, p, dist2=None):
    """(reach, from) of one (ny, nx) frame as reach_frame gives them, for frames of a million cells: a heap Dijkstra over flat lists with a
    border of impassable cells, then the from rule through `offers`.  tests/test_reach_cpu.py holds it to reach_frame on the small shapes."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    sx, sy = int(source[0]), int(source[1])
    t = terms_array(cost, (sx, sy), p, dist2)
    w = nx + 2
    T = np.pad(t, 1).ravel().tolist()
    inf = 1 << 62
    d = [inf] * len(T)
    s = (sy + 1) * w + sx + 1
    d[s] = 0
    heap = [(0, s)]
    push, pop = heapq.heappush, heapq.heappop
    edges = (-w, -1, 1, w)
    corners = ((-w - 1, -w, -1), (-w + 1, -w, 1), (w - 1, w, -1), (w + 1, w, 1))
    while heap:
        v, i = pop(heap)
        if v > d[i]:
            continue
        ti = T[i]
        for o in edges:
            tj = T[i + o]
            if tj:
                c = v + 5 * (ti + tj)
                if c < d[i + o]:
                    d[i + o] = c
                    push(heap, (c, i + o))
        for o, a, b in corners:
            tj = T[i + o]
            if tj and T[i + a] and T[i + b]:
                c = v + 7 * (ti + tj)
                if c < d[i + o]:
                    d[i + o] = c
                    push(heap, (c, i + o))
    r = np.array(d, np.int64).reshape(ny + 2, w)[1:-1, 1:-1]
    limit = p["max_reach"]
    r = np.where((r == inf) | ((limit > 0) & (r > limit)), NONE, r)
    assert r.max() <= NONE
    best, first = offers(t, r, limit)
    frm = from_of(first, (sx, sy))
    frm[r == NONE] = -1
    assert ((frm >= 0) == (r != NONE)).all(), "a reached cell without a predecessor"
    return r.astype(np.int32), frm.astype(np.int32)


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


def comb(ny, nx, pitch, gap, seed):
    """int8 costs 0 .. 99 with walls one cell thick across the image at x = pitch, 2 pitch .., each open for `gap` cells alternately at
    the bottom and at the top: the cheapest path from x = 0 to the far side runs the whole image back and forth."""
    c = np.random.default_rng(seed).integers(0, 100, (ny, nx)).astype(np.int8)
    for k, x in enumerate(range(pitch, nx - 1, pitch)):
        c[:, x] = 100
        if k % 2 == 0:
            c[ny - gap:, x] = 0
        else:
            c[:gap, x] = 0
    return c


def chain(reach, frm, source, tx, ty):
    """How a finished field of one frame uses the tiles of tx x ty cells: walks the from chain from the dearest cell back to the source
    (every hop to one of the 8 neighbours, onto a strictly smaller value) and returns a dict: `reached` cells; `every_tile`: each tile
    holds a reached cell; `tiles`: the chain's tiles in the order of the path, from the source outwards, without repeats in a row;
    `up` / `down`: how often the path passes into a tile of another word of 32 tiles with a larger / smaller index; `words`: the words
    it visits."""
    ny, nx = reach.shape
    tiles_x, tiles_y = (nx + tx - 1) // tx, (ny + ty - 1) // ty
    got = reach != NONE
    yy, xx = np.nonzero(got)
    seen = np.zeros(tiles_x * tiles_y, bool)
    seen[(yy // ty) * tiles_x + xx // tx] = True
    r, f = reach.ravel().tolist(), frm.ravel().tolist()
    i = int(np.argmax(np.where(got, reach, -1)))
    end = int(source[1]) * nx + int(source[0])
    tiles = []
    hops = 0
    while True:
        q = (i // nx // ty) * tiles_x + i % nx // tx
        if not tiles or tiles[-1] != q:
            tiles.append(q)
        if i == end:
            break
        j = f[i]
        assert 0 <= j < nx * ny and r[j] < r[i] and max(abs(j // nx - i // nx), abs(j % nx - i % nx)) == 1, "from of cell %d is %d" % (i, j)
        i, hops = j, hops + 1
        assert hops < nx * ny
    tiles.reverse()
    w = [q >> 5 for q in tiles]
    return dict(reached=int(got.sum()), every_tile=bool(seen.all()), tiles=tiles, hops=hops, words=sorted(set(w)),
                up=sum(1 for a, b in zip(w, w[1:]) if b > a), down=sum(1 for a, b in zip(w, w[1:]) if b < a))
