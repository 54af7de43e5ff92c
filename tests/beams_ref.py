"""The per-beam free space (pwpp_rasterize_beams, pwpp_beam_grid) restated by the rules of include/pwpp.h: a brute force from the
closed form of the digital line, vectorised over the beams per step k, in exact int64 (every product < 2^37).  Two ways in: from the
endpoint images (beams_of, beams_frames), and per POINT from a raw cloud (ends_of_points, beams_of_points) -- the theorem of the header
says both give the same two images.  It shares no code with the library.  Shared by tests/test_beams_cpu.py and
tests/test_gpu_beams.py."""
import math

import numpy as np

FREE, OCCUPIED, UNKNOWN = 0, 100, -1
NO_HEIGHT = -2 ** 31
INT32_MAX = 2 ** 31 - 1
R = 1 << 20
EYE_MAX = 1 << 30
GROUND, NONGROUND = 1, 2


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


def height(eye, z, k, n):
    """pwpp_beam_height: eye + ceil(clamp(z - eye, -R, R) * D / 2n), D = 2k - 1 where the rise is negative, else 2k + 1.  Python integers."""
    r = min(max(int(z) - int(eye), -R), R)
    D = 2 * k - 1 if r < 0 else 2 * k + 1
    return int(eye) - ((-(r * D)) // (2 * n))


def _trace(shape, origin, ex, ey, w, z, max_range):
    """(passes as int64 sums, low as int64 with INT64 max where nothing passed) of the beams into the cells (ex, ey) with weights w and heights z."""
    ny, nx = shape
    ox, oy, eye = (int(v) for v in origin)
    assert 0 <= ox < nx and 0 <= oy < ny and abs(eye) <= EYE_MAX
    passes = np.zeros((ny, nx), np.int64)
    low = np.full((ny, nx), np.iinfo(np.int64).max, np.int64)
    ex, ey, w, z = (np.asarray(a, np.int64).reshape(-1) for a in (ex, ey, w, z))
    dx, dy = ex - ox, ey - oy
    ax, ay, sx, sy = np.abs(dx), np.abs(dy), np.sign(dx), np.sign(dy)
    n = np.maximum(ax, ay)
    last = n - 1                                   # the interior points P_1 .. P_{n-1}
    if max_range > 0:
        last = np.minimum(last, max_range)
    r = np.clip(z - eye, -R, R)
    k = 0
    live = np.nonzero(last >= 1)[0]
    while len(live):
        k += 1
        nl = n[live]
        x = ox + sx[live] * ((2 * k * ax[live] + nl) // (2 * nl))
        y = oy + sy[live] * ((2 * k * ay[live] + nl) // (2 * nl))
        assert (np.maximum(np.abs(x - ox), np.abs(y - oy)) == k).all()           # P_k lies k cells from the origin (Chebyshev)
        D = np.where(r[live] < 0, 2 * k - 1, 2 * k + 1)
        h = eye - ((-(r[live] * D)) // (2 * nl))                                 # exact ceiling
        np.add.at(passes, (y, x), w[live])
        np.minimum.at(low, (y, x), h)
        live = live[last[live] > k]
    return passes, low


def _finish(passes, low):
    p = (passes % (1 << 32)).astype(np.uint32)
    return p, np.where(p == 0, NO_HEIGHT, low).astype(np.int64).astype(np.int32)


def beams_of(hits, zmin, origin, max_range=0):
    """(passes uint32, low int32) of ONE frame from its (ny, nx) endpoint images.  origin: (ox, oy, eye)."""
    hits, zmin = np.asarray(hits, np.int64), np.asarray(zmin, np.int64)
    ey, ex = np.nonzero((hits >= 1) & (zmin != NO_HEIGHT))
    return _finish(*_trace(hits.shape, origin, ex, ey, hits[ey, ex], zmin[ey, ex], max_range))


def occupancy_of(passes, low, target=None, occupancy_in=None, min_pass=1, clearance=0):
    """The byte of every cell: free iff the base byte is unknown, passes >= min_pass (unsigned) and, with a target, the target has a
    height and low - target <= clearance; else the base byte."""
    passes, low = np.asarray(passes).astype(np.int64), np.asarray(low, np.int64)
    base = np.full(passes.shape, UNKNOWN, np.int8) if occupancy_in is None else np.asarray(occupancy_in, np.int8)
    ok = (base == UNKNOWN) & (passes >= int(min_pass))
    if target is not None:
        t = np.asarray(target, np.int64)
        ok &= (t != NO_HEIGHT) & (low - t <= int(clearance))
    return np.where(ok, FREE, base).astype(np.int8)


def beams_frames(hits, zmin, origins, target=None, occupancy_in=None, max_range=0, min_pass=1, clearance=0):
    """What pwpp_beam_grid returns for (frames, ny, nx) images: (passes, low, occupancy).  origins: (ox, oy, eye) or one per frame."""
    hits = np.asarray(hits, np.int32)
    origins = np.asarray(origins, np.int64).reshape(-1, 3)
    if len(origins) == 1:
        origins = origins.repeat(len(hits), 0)
    out = [beams_of(hits[f], np.asarray(zmin)[f], origins[f], max_range) for f in range(len(hits))]
    passes, low = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return passes, low, occupancy_of(passes, low, target, occupancy_in, min_pass, clearance)


def _cells_of_points(xyz, grid):
    """(ix, iy, units(z)) of the float32 points that have a cell of the grid (x0, y0, cell, nx, ny) and a z: the cell rule of the
    obstacle raster, u = (c - c0) / cell in double, inside iff 0 <= u < n."""
    x0, y0, cell, nx, ny = grid
    p = np.asarray(xyz, np.float32)[:, :3].astype(np.float64)
    with np.errstate(invalid="ignore"):
        u, v = (p[:, 0] - float(x0)) / float(cell), (p[:, 1] - float(y0)) / float(cell)
        keep = (u >= 0.0) & (u < float(nx)) & (v >= 0.0) & (v < float(ny)) & ~np.isnan(p[:, 2])
    return np.floor(u[keep]).astype(np.int64), np.floor(v[keep]).astype(np.int64), units_image(p[keep, 2]).astype(np.int64)


def ends_of_points(xyz, grid):
    """(hits, zmin) of ONE frame's selected points: what pwpp_rasterize_beams gives for them."""
    nx, ny = int(grid[3]), int(grid[4])
    ix, iy, z = _cells_of_points(xyz, grid)
    hits = np.zeros((ny, nx), np.int64)
    zmin = np.full((ny, nx), np.iinfo(np.int64).max, np.int64)
    np.add.at(hits, (iy, ix), 1)
    np.minimum.at(zmin, (iy, ix), z)
    return hits.astype(np.int32), np.where(hits == 0, NO_HEIGHT, zmin).astype(np.int64).astype(np.int32)


def beams_of_points(xyz, grid, origin, max_range=0):
    """(passes, low) of ONE frame with every POINT's beam traced on its own, from its own cell and its own z."""
    nx, ny = int(grid[3]), int(grid[4])
    ix, iy, z = _cells_of_points(xyz, grid)
    return _finish(*_trace((ny, nx), origin, ix, iy, np.ones(len(ix), np.int64), z, max_range))


def random_ends(shape, eye, seed, fill=0.3, none=0.1):
    """(hits, zmin) int32 images: `fill` of the cells hold 1 .. 5 hits; a tenth of ALL cells have no zmin, the others heights with
    rises over `eye` from small to beyond +-R."""
    rng = np.random.default_rng(seed)
    hits = np.where(rng.random(shape) < fill, rng.integers(1, 6, shape), 0).astype(np.int32)
    kind = rng.integers(0, 4, shape)
    rise = np.where(kind == 0, rng.integers(-40, 41, shape),
                    np.where(kind == 1, rng.integers(-3000, 3001, shape),
                             np.where(kind == 2, rng.integers(-R - 5, R + 6, shape), rng.choice([-R - 1, -R, R, R + 1, 3 * R, -3 * R], shape))))
    zmin = np.where(rng.random(shape) < none, NO_HEIGHT, int(eye) + rise).astype(np.int32)
    return hits, zmin
