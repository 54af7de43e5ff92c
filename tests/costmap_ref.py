"""The costmap rule of include/pwpp.h restated in numpy, from the header's words and not from the C++: three layers, each a value
0 .. 100 or unknown, folded by a maximum; the inflation is a table of bytes indexed by dist2.  The reference of the CPU and GPU
tests of pwpp_costmap_grid, pwpp_costmap_obstacles and pwpp_costmap_cell."""
import numpy as np

OCCUPANCY, INFLATION, TERRAIN, WHY_UNKNOWN = 1, 2, 4, 8
OCC_FREE, OCC_OCCUPIED = 0, 100
DIST_BEYOND = 0x7FFFFFFF
MAX_CURVE = 4097


def fold(layers, occupancy_unknown, terrain_unknown, unknown_below, curve=None, o=None, t=None, d=None):
    """(cost int8, why uint8) of the images o (int8), t (int8), d (int32) of one shape -- each needed only with its layer -- under
    the four parameters and the uint8 table `curve`."""
    shape = next(np.shape(a) for a in (o, t, d) if a is not None)
    known, unknown = [], np.zeros(shape, bool)  # known: (bit, value as int64, mask of the cells where the layer has a value)
    if layers & OCCUPANCY:
        o = np.asarray(o, np.int8).astype(np.int64)
        value = np.where(o == OCC_OCCUPIED, 100, 0)
        has = (o == OCC_OCCUPIED) | (o == OCC_FREE)
        if occupancy_unknown >= 0:
            value, has = np.where(has, value, occupancy_unknown), np.ones(shape, bool)
        known.append((OCCUPANCY, value, has))
        unknown |= ~has
    if layers & INFLATION:
        table = np.asarray(curve, np.uint8).astype(np.int64)
        index = np.asarray(d, np.int32).astype(np.int64) & 0xFFFFFFFF  # (the word as a uint32)
        inside = index < len(table)
        value = np.where(inside, table[np.where(inside, index, 0)], 0)
        known.append((INFLATION, value, np.ones(shape, bool)))
    if layers & TERRAIN:
        t = np.asarray(t, np.int8).astype(np.int64)
        value, has = np.minimum(t, 100), t >= 0
        if terrain_unknown >= 0:
            value, has = np.where(has, value, terrain_unknown), np.ones(shape, bool)
        known.append((TERRAIN, value, has))
        unknown |= ~has
    m = np.zeros(shape, np.int64)
    for _, value, has in known:
        m = np.maximum(m, np.where(has, value, 0))
    why = np.where(unknown, WHY_UNKNOWN, 0)
    for bit, value, has in known:
        why = why | np.where(has & (value == m) & (m > 0), bit, 0)
    cost = np.where(unknown & (m < unknown_below), -1, m)
    return cost.astype(np.int8), why.astype(np.uint8)


def cap(n_curve):
    """max_dist of the distances a call computes itself: max(1, R), R the least integer with R * R >= n_curve - 1."""
    r = 0
    while r * r < n_curve - 1:
        r += 1
    return max(1, r)


def dist2_brute(occupied, max_dist=0):
    """The exact squared distance of every cell of the (frames, ny, nx) boolean images to the nearest occupied cell of its frame,
    DIST_BEYOND where there is none or (max_dist > 0) the distance exceeds max_dist."""
    occupied = np.asarray(occupied, bool)
    frames, ny, nx = occupied.shape
    out = np.full(occupied.shape, DIST_BEYOND, np.int64)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for f in range(frames):
        for jy, jx in zip(*np.nonzero(occupied[f])):
            out[f] = np.minimum(out[f], (yy - jy) ** 2 + (xx - jx) ** 2)
    if max_dist > 0:
        out[out > max_dist * max_dist] = DIST_BEYOND
    return out.astype(np.int32)


def curve(cell, inscribed, radius, decay, peak):
    """The table of pwpp_costmap_curve with numpy's exp: every entry may differ by 1 from the C library's."""
    n = 1
    while np.sqrt(float(n)) * cell <= radius:
        n += 1
    r = np.sqrt(np.arange(n, dtype=np.float64)) * cell
    return np.where(r <= inscribed, 100, np.floor(peak * np.exp(-decay * (r - inscribed)))).astype(np.int64)
