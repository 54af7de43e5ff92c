"""The obstacle distances (pwpp_distance_grid) restated by the rules of include/pwpp.h: a brute force that follows the
definition -- per cell the minimum over ALL occupied cells of the 64-bit key (squared distance << 32 | cell index), so the
smallest index wins among several nearest cells -- a second, separable restatement (nearest occupied column per row, then the
minimum over the rows) to check the first against, the cap applied to an unlimited result, and the shapes both test files run.
Shared by tests/test_obstacle_distance_cpu.py and tests/test_gpu_obstacle_distance.py."""
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


def separable(count, min_count=1):
    """The second restatement: (dist2, nearest) from the rows' nearest columns and the minimum of the key over the rows."""
    count = np.asarray(count, np.int32)
    ny, nx = count.shape
    gx = row_nearest(count >= min_count)
    ix = np.arange(nx, dtype=np.int64)[None, None, :]
    iy = np.arange(ny, dtype=np.int64)[:, None, None]
    jy = np.arange(ny, dtype=np.int64)[None, :, None]
    g = gx[None, :, :]
    keys = np.where(g >= 0, (((g - ix) ** 2 + (iy - jy) ** 2) << 32) | (jy * nx + g), KEY_NONE).min(axis=1)  # [iy][jy][ix] -> [iy][ix]
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
