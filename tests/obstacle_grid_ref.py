"""The obstacle grid (pwpp_rasterize_obstacles) restated in numpy by the rules of include/pwpp.h: given the coordinates of a
frame's non-ground points and the ground sample of each (pwpp_query_ground of the point's own position, or its restatement
tests/ground_query_ref.py), the three images count, top and unref.  Shared by tests/test_obstacle_grid_cpu.py and
tests/test_gpu_obstacle_grid.py."""
import numpy as np

from ground_query_ref import HIDDEN_DECISIONS

F32 = np.float32
QNAN_BITS = 0x7FC00000


def height_keys(h):
    """The monotone uint32 key of float32 heights: ascending keys = ascending heights, with -0.0 below +0.0.  No height has key 0
    but the NaN 0xffffffff, which is never counted: 0 means "empty"."""
    b = np.ascontiguousarray(h, F32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def heights_of_keys(k):
    """The inverse of height_keys; key 0 becomes the quiet NaN."""
    k = np.ascontiguousarray(k, np.uint32)
    b = np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return np.where(k == 0, np.uint32(QNAN_BITS), b).astype(np.uint32).view(F32)


def cells_of(c, c0, cell, n):
    """(kept, index): u = ((double)c - c0) / cell, kept iff 0 <= u < n (a NaN is not), index = floor(u)."""
    with np.errstate(all="ignore"):
        u = (np.ascontiguousarray(c, F32).astype(np.float64) - np.float64(c0)) / np.float64(cell)
        kept = (u >= 0.0) & (u < float(n))
    idx = np.zeros(len(u), np.int64)
    idx[kept] = np.floor(u[kept]).astype(np.int64)
    return kept, idx


def restate_obstacles(xyz, samples, x0, y0, cell, nx, ny, h_min, h_max, ground_only=False):
    """(count int32, top float32, unref int32), each (ny, nx), of the points `xyz` (m, 3) with ground samples `samples` (m,)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    assert len(samples) == len(xyz)
    kx, ix = cells_of(xyz[:, 0], x0, cell, nx)
    ky, iy = cells_of(xyz[:, 1], y0, cell, ny)
    inside = kx & ky
    o = iy * nx + ix
    noref = samples["patch"] < 0
    if ground_only:
        noref = noref | np.isin(samples["decision"], HIDDEN_DECISIONS)
    hgt = np.ascontiguousarray(samples["distance"], F32)
    with np.errstate(invalid="ignore"):
        counted = inside & ~noref & (F32(h_min) <= hgt) & (hgt <= F32(h_max))  # (float32 compares; a NaN height fails both)
    count = np.zeros(nx * ny, np.int32)
    unref = np.zeros(nx * ny, np.int32)
    keys = np.zeros(nx * ny, np.uint32)
    np.add.at(count, o[counted], 1)
    np.add.at(unref, o[inside & noref], 1)
    np.maximum.at(keys, o[counted], height_keys(hgt[counted]))
    return count.reshape(ny, nx), heights_of_keys(keys).reshape(ny, nx), unref.reshape(ny, nx)


def same_images(a, b):
    """Bit-equal images; for float images NaNs compare as NaN-ness (the library writes the quiet NaN 0x7fc00000)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != F32:
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))
