"""The obstacle distances (pwpp_distance_grid) restated by the rules of include/pwpp.h: a brute force that follows the
definition -- per cell the minimum over ALL occupied cells of the 64-bit key (squared distance << 32 | cell index), so the
smallest index wins among several nearest cells -- a second, separable restatement (nearest occupied column per row, then the
minimum over the rows) to check the first against, the cap applied to an unlimited result, and the shapes both test files run.
Shared by tests/test_obstacle_distance_cpu.py and tests/test_gpu_obstacle_distance.py."""
import functools

import numpy as np

from obstacle_clusters_ref import PATTERNS, pattern  # noqa: F401  (the pattern set of the clusters)
from obstacle_clusters_ref import SHAPES as CLUSTER_SHAPES

BEYOND = 0x7fffffff
KEY_NONE = np.int64(0x7fffffffffffffff)  # dist2 BEYOND, nearest -1 (the low half all ones)
LDS_ROWS = 512  # the tallest strip the library's column pass keeps in LDS: the shapes aim at both sides of it
# (nx, ny): the clusters' shapes; a column taller than any LDS strip; two rows of three 64-column chunks; the LDS limit and one beyond
SHAPES = CLUSTER_SHAPES + [(5, 700), (130, 2), (4, LDS_ROWS), (5, LDS_ROWS + 1)]
MAX_DISTS = (0, 1, 2, 5)


def split(keys):
    """(dist2, nearest) int32 of int64 keys."""
    return (keys >> 32).astype(np.int32), (keys & 0xffffffff).astype(np.uint32).view(np.int32)


def brute_force(count, min_count=1, chunk=256):
    """(dist2, nearest), both (ny, nx) int32, of ONE frame by the definition; unlimited."""
    count = np.asarray(count, np.int32)
    ny, nx = count.shape
    jy, jx = np.nonzero(count >= min_count)
    if len(jy) == 0:
        return np.full((ny, nx), BEYOND, np.int32), np.full((ny, nx), -1, np.int32)
    jy, jx = jy.astype(np.int64), jx.astype(np.int64)
    low = jy * nx + jx
    cells = np.arange(nx * ny, dtype=np.int64)
    keys = np.empty(nx * ny, np.int64)
    for a in range(0, nx * ny, chunk):  # (chunk x occupied keys at a time)
        iy, ix = cells[a:a + chunk, None] // nx, cells[a:a + chunk, None] % nx
        keys[a:a + chunk] = ((((ix - jx) ** 2 + (iy - jy) ** 2) << 32) | low).min(axis=1)
    d2, near = split(keys)
    return d2.reshape(ny, nx), near.reshape(ny, nx)


def row_nearest(occ):
    """gx (ny, nx) int64: the nearest occupied column of every cell's own row, the left one on a tie, -1 where the row has none."""
    ny, nx = occ.shape
    x = np.arange(nx, dtype=np.int64)[None, :].repeat(ny, 0)
    left = np.maximum.accumulate(np.where(occ, x, -1), axis=1)
    right = np.minimum.accumulate(np.where(occ, x, 2 * nx)[:, ::-1], axis=1)[:, ::-1]
    take_left = (left >= 0) & ((right >= nx) | (x - left <= right - x))
    return np.where(take_left, left, np.where(right < nx, right, -1))


def separable(count, min_count=1, block_bytes=32 << 20):
    """The second restatement: (dist2, nearest) from the rows' nearest columns and the minimum of the key over the rows.  The
    rows iy are taken in blocks whose [iy][jy][ix] int64 array stays below block_bytes."""
    count = np.asarray(count, np.int32)
    ny, nx = count.shape
    gx = row_nearest(count >= min_count)
    ix = np.arange(nx, dtype=np.int64)[None, None, :]
    jy = np.arange(ny, dtype=np.int64)[None, :, None]
    g = gx[None, :, :]
    low, none = jy * nx + g, g < 0
    dx2 = (g - ix) ** 2
    step = max(1, block_bytes // (8 * nx * ny))
    keys = np.empty((ny, nx), np.int64)
    for a in range(0, ny, step):
        iy = np.arange(a, min(ny, a + step), dtype=np.int64)[:, None, None]
        k = dx2 + (iy - jy) ** 2  # [iy][jy][ix]
        k <<= 32
        k |= low
        k[np.broadcast_to(none, k.shape)] = KEY_NONE
        keys[a:a + step] = k.min(axis=1)
    return split(keys)


def capped(result, max_dist):
    """What a call with max_dist reports, from the unlimited (dist2, nearest): beyond where the true dist2 exceeds max_dist^2."""
    d2, near = result
    if max_dist == 0:
        return d2, near
    far = d2.astype(np.int64) > max_dist * max_dist
    return np.where(far, BEYOND, d2).astype(np.int32), np.where(far, -1, near).astype(np.int32)


def metres_of(dist2, cell):
    """numpy's statement of the metres image: one square root and one multiply in double, one rounding to float; +inf beyond."""
    dist2 = np.asarray(dist2)
    d = (np.sqrt(dist2.astype(np.float64)) * cell).astype(np.float32)  # = np.float32(np.sqrt(np.float64(dist2)) * cell), for every shape
    return np.where(dist2 == BEYOND, np.float32(np.inf), d).astype(np.float32)


def distance_frames(count, min_count=1, max_dist=0):
    """What pwpp_distance_grid returns for a (frames, ny, nx) image: (dist2, nearest)."""
    out = [capped(brute_force(c, min_count), max_dist) for c in np.asarray(count, np.int32)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- the column pass's tilings: tall images of several strips ---------------------------------------------------------------------
STRIP, TALL_TILE = 64, 256  # columns of a strip; rows of a tile that is read from global memory
# (nx, ny).  At 64-row tiles 577 = 9 * 64 + 1 and 513 = 8 * 64 + 1: the last tile has one row.  130 columns: 3 strips, the last
# with 2 live lanes; 65: 2 strips, the last with 1.
TALL_SHAPES = [(130, 577), (65, 513)]
# no cap; the smallest; both sides of the change from a 384-row tile to one that is no multiple of 64; the two narrowest halo
# tilings (66 and 64 tile rows under 223 and 224 halo rows); the first cap without a halo tiling; the largest cap there is
TALL_MAX_DISTS = (0, 1, 64, 65, 223, 224, 225, 46340)


def plan(ny, max_dist, path=0):
    """(lds, tile_rows, halo, row_tiles) of the column pass, restated from the three regimes of its launcher:
    A  path 0, ny <= 512: the whole column in LDS, one tile;
    B  path 0, ny > 512, 1 <= max_dist <= 224: tiles of 512 - 2 * max_dist rows with max_dist rows either side in LDS;
    C  everything else (no cap or one of 225 and more on a tall image, and path 1 always): tiles of 256 rows from global memory."""
    if path == 0 and ny <= LDS_ROWS:
        lds, tile_rows, halo = 1, ny, 0
    elif path == 0 and 1 <= max_dist <= 224:
        lds, tile_rows, halo = 1, LDS_ROWS - 2 * max_dist, max_dist
    else:
        lds, tile_rows, halo = 0, TALL_TILE, 0
    return lds, tile_rows, halo, -(-ny // tile_rows)


def regime(ny, max_dist, path=0):
    lds, tile_rows, halo, _ = plan(ny, max_dist, path)
    return "C" if not lds else "B" if halo else "A"


TALL_PATTERNS = ["row_top", "row_bottom", "row_mid", "two_rows", "lattice", "columns", "corners", "sparse", "borders"]
TWO_ROWS = (92, 292)  # their midpoint 192 is a border of the 64-row tiling: both 100 rows away, the upper one wins through the halo
# the patterns with a closed form for the largest distance along a column, for the caps they make binding
AXIS_PATTERNS = ("row_top", "row_bottom", "row_mid", "two_rows", "lattice", "corners")


def lattice_cell(nx, ny):
    """(x, y) of the single cell of `lattice`: (65, 288) on 130 x 577, (32, 256) on 65 x 513."""
    return nx // 2, ny // 2


def tall_occupancy(name, nx, ny):
    """The boolean (ny, nx) pattern `name` of TALL_PATTERNS: all sparse, so that brute_force stays cheap."""
    occ = np.zeros((ny, nx), bool)
    if name == "row_top":
        occ[0] = True
    elif name == "row_bottom":
        occ[ny - 1] = True
    elif name == "row_mid":
        occ[ny // 2] = True
    elif name == "two_rows":
        occ[TWO_ROWS[0]] = occ[TWO_ROWS[1]] = True
    elif name == "lattice":
        x, y = lattice_cell(nx, ny)
        occ[y, x] = True
    elif name == "columns":  # horizontal distances only: gx from both sides, the left one on a tie
        occ[:, 0] = occ[:, nx - 1] = True
    elif name == "corners":
        occ[0, 0] = occ[0, nx - 1] = occ[ny - 1, 0] = occ[ny - 1, nx - 1] = True
    elif name == "sparse":  # early exit by the best so far
        occ = np.random.default_rng([7, nx, ny]).random((ny, nx)) < 0.003
    elif name == "borders":  # a cell either side of every tile border of every plan: the nearest cell is one row away, in the other tile
        for k, max_dist in enumerate(TALL_MAX_DISTS):  # (columns of its own for every cap: borders two rows apart do not shadow each other)
            _, tile_rows, _, row_tiles = plan(ny, max_dist)
            for t in range(1, row_tiles):
                occ[t * tile_rows - 1, 3 + 7 * k] = occ[t * tile_rows, nx - 4 - 7 * k] = True
    else:
        raise ValueError(name)
    return occ


def tall_pattern(name, nx, ny):
    """count (ny, nx) int32 of a tall pattern: 0 off the pattern, 1 and 2 on it, so that min_count 2 keeps a part of it -- the
    lower of two_rows, every other cell (x + y odd) of the others, a random half of `sparse`."""
    occ = tall_occupancy(name, nx, ny)
    y, x = np.mgrid[0:ny, 0:nx]
    two = (x + y) % 2 == 1
    if name == "two_rows":
        two = y == TWO_ROWS[1]
    elif name == "sparse":
        two = np.random.default_rng([8, nx, ny]).random((ny, nx)) < 0.5
    return np.where(occ, 1 + two, 0).astype(np.int32)


def farthest_along_a_column(name, nx, ny):
    """The largest distance of a cell to the pattern measured straight along its column, in closed form (min_count 1): the
    caps m < this are the ones the image can hold -- a cell m rows away and one m + 1 rows away both exist."""
    cy = lattice_cell(nx, ny)[1]
    return {"row_top": ny - 1, "row_bottom": ny - 1, "row_mid": max(ny // 2, ny - 1 - ny // 2),
            "two_rows": max(TWO_ROWS[0], (TWO_ROWS[1] - TWO_ROWS[0]) // 2, ny - 1 - TWO_ROWS[1]),
            "lattice": max(cy, ny - 1 - cy), "corners": (ny - 1) // 2}[name]


@functools.lru_cache(maxsize=None)
def tall_reference(name, nx, ny, min_count=1):
    """(count, dist2, nearest) of a tall pattern, unlimited, by the brute force: computed once, shared, never written."""
    count = tall_pattern(name, nx, ny)
    dist2, nearest = brute_force(count, min_count)
    for a in (count, dist2, nearest):
        a.setflags(write=False)
    return count, dist2, nearest
