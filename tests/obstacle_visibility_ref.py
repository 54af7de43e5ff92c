"""The line-of-sight free space (pwpp_visibility_grid) restated by the rules of include/pwpp.h: a brute force from the closed form
of the digital line, P_k = o + sgn(d) * ((2k|d| + n) // (2n)) per axis, vectorised over the cells per step k -- every point from
its own division, nothing carried from step to step but the previous point -- with the rules (a) and (b), the cap, and the
statement first -> occupancy.  It shares no code with the library.  `cells` evaluates a given list of cells only (the large
images).  Shared by tests/test_obstacle_visibility_cpu.py and tests/test_gpu_obstacle_visibility.py."""
import numpy as np

NONE, BEYOND = -1, -2
FREE, OCCUPIED, UNKNOWN = 0, 100, -1


def first_of(count, origin, min_count=1, max_range=0, cells=None, rule_a=True):
    """first of ONE frame: the (ny, nx) int32 image, or with cells = an (m, 2) array of (cx, cy) the m values of those cells.
    rule_a=False leaves rule (a) out: what the tests of the watertight ring discriminate against."""
    occ = np.asarray(count) >= min_count
    ny, nx = occ.shape
    ox, oy = int(origin[0]), int(origin[1])
    assert 0 <= ox < nx and 0 <= oy < ny
    if cells is None:
        cy, cx = (a.reshape(-1).astype(np.int64) for a in np.mgrid[0:ny, 0:nx])
    else:
        cells = np.asarray(cells, np.int64).reshape(-1, 2)
        cx, cy = cells[:, 0], cells[:, 1]
    dx, dy = cx - ox, cy - oy
    ax, ay = np.abs(dx), np.abs(dy)
    sx, sy = np.sign(dx), np.sign(dy)
    n = np.maximum(ax, ay)
    first = np.full(len(cx), NONE, np.int64)
    here = n == 0
    first[here] = np.where(occ[cy[here], cx[here]], cy[here] * nx + cx[here], NONE)
    beyond = (n > max_range) if max_range > 0 else np.zeros(len(cx), bool)
    first[beyond] = BEYOND
    live = np.nonzero(~here & ~beyond)[0]  # the cells still walking
    px, py = np.full(len(live), ox, np.int64), np.full(len(live), oy, np.int64)
    k = 0
    while len(live):
        k += 1
        nl = n[live]
        x = ox + sx[live] * ((2 * k * ax[live] + nl) // (2 * nl))
        y = oy + sy[live] * ((2 * k * ay[live] + nl) // (2 * nl))
        assert (np.abs(x - px) <= 1).all() and (np.abs(y - py) <= 1).all()
        squeezed = (x != px) & (y != py) & occ[y, px] & occ[py, x] if rule_a else np.zeros(len(live), bool)
        hit = ~squeezed & occ[y, x]
        first[live[squeezed]] = np.minimum(y * nx + px, py * nx + x)[squeezed]
        first[live[hit]] = (y * nx + x)[hit]
        done = squeezed | hit | (nl == k)
        assert ((x == cx[live]) & (y == cy[live]))[nl == k].all()  # P_n = c
        live, px, py = live[~done], x[~done], y[~done]
    first = first.astype(np.int32)
    return first.reshape(ny, nx) if cells is None else first


def occupancy_of(count, first, min_count=1, cells=None):
    """The byte of every cell: occupied where it holds returns, seen or not; free where the line is clear; unknown otherwise."""
    occ = np.asarray(count) >= min_count
    if cells is not None:
        cells = np.asarray(cells, np.int64).reshape(-1, 2)
        occ = occ[cells[:, 1], cells[:, 0]]
    return np.where(occ, OCCUPIED, np.where(np.asarray(first) == NONE, FREE, UNKNOWN)).astype(np.int8)


def capped(first, origin, max_range):
    """What a call with max_range reports, from the unlimited first image of one frame."""
    if max_range == 0:
        return first
    ny, nx = first.shape
    iy, ix = np.mgrid[0:ny, 0:nx]
    n = np.maximum(np.abs(ix - int(origin[0])), np.abs(iy - int(origin[1])))
    return np.where(n > max_range, BEYOND, first).astype(np.int32)


def visibility_frames(count, origins, min_count=1, max_range=0):
    """What pwpp_visibility_grid returns for a (frames, ny, nx) image: (first, occupancy).  origins: (ox, oy) or one per frame."""
    count = np.asarray(count, np.int32)
    origins = np.asarray(origins, np.int64).reshape(-1, 2)
    if len(origins) == 1:
        origins = origins.repeat(len(count), 0)
    first = np.stack([first_of(c, o, min_count, max_range) for c, o in zip(count, origins)])
    return first, occupancy_of(count, first, min_count)


def random_count(nx, ny, fill, min_count, seed):
    """A count image whose cells are occupied (>= min_count) with probability `fill`, the others below min_count."""
    rng = np.random.default_rng(seed)
    occ = rng.random((ny, nx)) < fill
    return np.where(occ, min_count + rng.integers(0, 3, (ny, nx)), rng.integers(0, min_count, (ny, nx))).astype(np.int32)


def ring_image(size=41, centre=(20, 20), radius=12):
    """The thin 8-connected boundary of a disc: the disc's cells that have a 4-neighbour outside it.  Returns (count, disc)."""
    iy, ix = np.mgrid[0:size, 0:size]
    disc = (ix - centre[0]) ** 2 + (iy - centre[1]) ** 2 <= radius * radius
    p = np.pad(disc, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return (disc & ~inner).astype(np.int32), disc


RING_ORIGINS = ((20, 20), (15, 23), (27, 14))
