"""The viewshed (pwpp_viewshed_grid) restated by the rules of include/pwpp.h: a brute force from the closed form of the digital
line, vectorised over the cells per step k, that meets EVERY blocker of every line -- nothing stops early -- and keeps, per cell, the
nearest blocker that hides, whether one was opaque, and the largest ceil(r * 2n / D) in exact int64 (every product < 2^38).  It
shares no code with the library.  `cells` evaluates a given list of cells only (the large images).  Shared by
tests/test_viewshed_cpu.py and tests/test_gpu_viewshed.py."""
import math

import numpy as np

NONE, BEYOND = -1, -2
FREE, OCCUPIED, UNKNOWN = 0, 100, -1
NO_HEIGHT = -2 ** 31
INT32_MAX = 2 ** 31 - 1
R = 1 << 20
UNITS_PER_M = 1024
OPAQUE = 1 << 40    # above every rise
BELOW = -(1 << 40)  # under every rise


def units(metres):
    """pwpp_viewshed_units of one value."""
    v = float(metres)
    if math.isnan(v):
        return NO_HEIGHT
    return int(math.floor(min(max(v * 1024.0, -2.0 ** 30), 2.0 ** 30) + 0.5))


def units_image(a):
    """pwpp_viewshed_units of every element of a float64 array."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore"):
        q = np.floor(np.clip(a * 1024.0, -2.0 ** 30, 2.0 ** 30) + 0.5)
    return np.where(np.isnan(a), float(NO_HEIGHT), q).astype(np.int64).astype(np.int32)


def _rise(img, eye):
    """clamp(height - eye, -R, R) in int64; None where there is no image."""
    return None if img is None else np.clip(np.asarray(img, np.int64) - int(eye), -R, R)


def viewshed_of(count, origin, block=None, target=None, min_count=1, max_range=0, cells=None):
    """(first, shadow, hidden_rise) of ONE frame: (ny, nx) images, or with cells = an (m, 2) array of (cx, cy) their m values.
    origin: (ox, oy, eye).  hidden_rise is the target rise of every cell as an int64 (BELOW: minus infinity): what the theorem
    compares with shadow - eye."""
    occ = np.asarray(count) >= min_count
    ny, nx = occ.shape
    ox, oy, eye = (int(v) for v in origin)
    assert 0 <= ox < nx and 0 <= oy < ny and eye != NO_HEIGHT
    no_b = np.ones((ny, nx), bool) if block is None else np.asarray(block) == NO_HEIGHT
    rb = np.where(no_b, OPAQUE, 0 if block is None else _rise(block, eye))      # the rise of a cell as a blocker (read where occupied)
    no_t = np.ones((ny, nx), bool) if target is None else np.asarray(target) == NO_HEIGHT
    rt = np.where(occ, np.where(no_b, BELOW, rb), np.where(no_t, BELOW, 0 if target is None else _rise(target, eye)))
    if cells is None:
        cy, cx = (a.reshape(-1).astype(np.int64) for a in np.mgrid[0:ny, 0:nx])
    else:
        cells = np.asarray(cells, np.int64).reshape(-1, 2)
        cx, cy = cells[:, 0], cells[:, 1]
    m = len(cx)
    dx, dy = cx - ox, cy - oy
    ax, ay, sx, sy = np.abs(dx), np.abs(dy), np.sign(dx), np.sign(dy)
    n = np.maximum(ax, ay)
    t = rt[cy, cx]
    beyond = (n > max_range) if max_range > 0 else np.zeros(m, bool)
    hider = np.full(m, -1, np.int64)           # the reported cell of the nearest blocker that hides
    any_b, dark = np.zeros(m, bool), np.zeros(m, bool)
    cast = np.full(m, -(1 << 62), np.int64)    # max ceil(r * 2n / D) over the blockers that are not opaque

    def meet(idx, r, D, cell):
        """the blockers (r, D, cell) of the cells idx (all arrays of one length)"""
        tt, n2 = t[idx], 2 * n[idx]
        opaque = r >= OPAQUE
        rr = np.where(opaque, 0, r)
        hides = opaque | (tt <= BELOW) | (rr * n2 > np.where(tt <= BELOW, 0, tt) * D)
        new = hides & (hider[idx] < 0)
        hider[idx[new]] = cell[new]
        any_b[idx] = True
        dark[idx[opaque]] = True
        c = -((-(rr * n2)) // D)               # exact ceiling
        fin = ~opaque
        cast[idx[fin]] = np.maximum(cast[idx[fin]], c[fin])

    live = np.nonzero((n > 0) & ~beyond)[0]
    px, py = np.full(len(live), ox, np.int64), np.full(len(live), oy, np.int64)
    k = 0
    while len(live):
        k += 1
        nl = n[live]
        x = ox + sx[live] * ((2 * k * ax[live] + nl) // (2 * nl))
        y = oy + sy[live] * ((2 * k * ay[live] + nl) // (2 * nl))
        assert (np.abs(x - px) <= 1).all() and (np.abs(y - py) <= 1).all()
        a = (x != px) & (y != py) & occ[y, px] & occ[py, x]                    # rule (a): A = (px, y), B = (x, py)
        if a.any():
            ia, ib = (y * nx + px)[a], (py * nx + x)[a]
            ra, rbb = rb[y, px][a], rb[py, x][a]
            r = np.minimum(ra, rbb)
            cell = np.where(ra < rbb, ia, np.where(rbb < ra, ib, np.minimum(ia, ib)))
            meet(live[a], r, np.full(a.sum(), 2 * k - 1, np.int64), cell)
        b = (nl > k) & occ[y, x]                                                 # rule (b), k < n only
        if b.any():
            meet(live[b], rb[y, x][b], np.full(b.sum(), 2 * k, np.int64), (y * nx + x)[b])
        done = nl == k
        assert ((x == cx[live]) & (y == cy[live]))[done].all()                   # P_n = c
        live, px, py = live[~done], x[~done], y[~done]
    first = np.where(hider >= 0, hider, np.where(occ[cy, cx], cy * nx + cx, NONE))
    first = np.where(beyond, BEYOND, first).astype(np.int32)
    shadow = np.where(dark, INT32_MAX, np.clip(eye + np.clip(cast, -R, R + 1), -INT32_MAX, INT32_MAX - 1))
    shadow = np.where(any_b & ~beyond, shadow, NO_HEIGHT).astype(np.int32)
    if cells is None:
        return first.reshape(ny, nx), shadow.reshape(ny, nx), t.reshape(ny, nx)
    return first, shadow, t


def occupancy_of(count, first, seen=None, min_count=1, min_seen=1, cells=None):
    """The byte of every cell: occupied; else free where witnessed; else free where first is NONE; else unknown."""
    occ = np.asarray(count) >= min_count
    wit = np.zeros(occ.shape, bool) if seen is None else np.asarray(seen) >= min_seen
    if cells is not None:
        cells = np.asarray(cells, np.int64).reshape(-1, 2)
        occ, wit = occ[cells[:, 1], cells[:, 0]], wit[cells[:, 1], cells[:, 0]]
    return np.where(occ, OCCUPIED, np.where(wit | (np.asarray(first) == NONE), FREE, UNKNOWN)).astype(np.int8)


def viewshed_frames(count, origins, block=None, target=None, seen=None, min_count=1, min_seen=1, max_range=0):
    """What pwpp_viewshed_grid returns for (frames, ny, nx) images: (first, shadow, occupancy).  origins: (ox, oy, eye) or one per frame."""
    count = np.asarray(count, np.int32)
    origins = np.asarray(origins, np.int64).reshape(-1, 3)
    if len(origins) == 1:
        origins = origins.repeat(len(count), 0)
    pick = lambda a, f: None if a is None else np.asarray(a)[f]
    out = [viewshed_of(count[f], origins[f], pick(block, f), pick(target, f), min_count, max_range)[:2] for f in range(len(count))]
    first, shadow = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return first, shadow, occupancy_of(count, first, seen, min_count, min_seen)


def hidden_of(count, first, min_count=1):
    """Whether a blocker hides the cell: first names another cell."""
    ny, nx = np.asarray(count).shape[-2:]
    own = np.arange(ny * nx).reshape(ny, nx)
    return (np.asarray(first) >= 0) & (np.asarray(first) != own)


def random_heights(shape, eye, seed, none=0.1):
    """An int32 height image: a tenth NO_HEIGHT, the others with rises over `eye` from small to beyond +-R."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 4, shape)
    rise = np.where(kind == 0, rng.integers(-40, 41, shape),
                    np.where(kind == 1, rng.integers(-3000, 3001, shape),
                             np.where(kind == 2, rng.integers(-R - 5, R + 6, shape), rng.choice([-R - 1, -R, R, R + 1, 3 * R, -3 * R], shape))))
    return np.where(rng.random(shape) < none, NO_HEIGHT, int(eye) + rise).astype(np.int32)


def kerb_row(length=40):
    """Theorem 4's scene: (count, block, target, origin) of one row."""
    count = np.zeros((1, length), np.int32)
    count[0, 4] = 1
    block = np.full((1, length), NO_HEIGHT, np.int32)
    block[0, 4] = 1500
    return count, block, np.zeros((1, length), np.int32), (0, 0, 1700)
