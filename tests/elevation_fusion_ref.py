"""The contract of the elevation fusion (pwpp_fuse_height_grid, include/pwpp.h) restated in numpy double and integers: vectorised
over the map's cells, looping over the frames in order, sharing no code with the library.  numpy on x86-64 forms no FMA, divides in
IEEE and rounds ties to even, so what the library computes must EQUAL this: no tolerance appears anywhere.

    grid  (x0, y0, cell) of the frame images, whose shape gives nx and ny          pose  {a, b, tx, c, d, ty}, map-from-frame
    mgrid (X0, Y0, CELL, NX, NY) of the maps                                         n_max the observations a mean remembers
"""
import numpy as np

M = 1 << 20  # |q| of one observation: 1024 m in units of 2^-10 m
NAN_BITS = 0x7FC00000
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def update(s, n, q, n_max):
    """The update of one cell in Python integers: (sum, n) after the observation q."""
    if n < n_max:
        return s + q, n + 1
    share = abs(s) // n  # C's division truncates toward zero
    return s - (share if s >= 0 else -share) + q, n


def observe(image, grid, pose, tz, mgrid):
    """(observed, q) of every map cell in one frame: the height under the cell's centre plus tz, in units of 2^-10 m."""
    x0, y0, cell = (np.float64(v) for v in grid)
    ny, nx = image.shape
    X0, Y0, CELL, NX, NY = mgrid
    a, b, tx, c, d, ty = (np.float64(v) for v in pose)
    jy, jx = np.mgrid[0:NY, 0:NX]
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.float64(X0) + (jx.astype(np.float64) + 0.5) * np.float64(CELL)
        my = np.float64(Y0) + (jy.astype(np.float64) + 0.5) * np.float64(CELL)
        dx = mx - tx
        dy = my - ty
        fx = a * dx + c * dy
        fy = b * dx + d * dy
        u = (fx - x0) / cell
        v = (fy - y0) / cell
        inside = (u >= 0) & (u < nx) & (v >= 0) & (v < ny)  # (a NaN compares false)
        ix = np.where(inside, np.floor(np.where(inside, u, 0.0)), 0).astype(np.int64)
        iy = np.where(inside, np.floor(np.where(inside, v, 0.0)), 0).astype(np.int64)
        Z = image[iy, ix].astype(np.float64) + np.float64(tz)
        seen = inside & np.isfinite(Z) & (np.abs(Z) <= 1024.0)
        q = np.rint(np.where(seen, Z, 0.0) * 1024.0).astype(np.int64)
    return seen, q


def shifted(sum_in, n_in, mgrid, n_maps, shift, n_max):
    """The start of every cell: the shifted inputs, normalised."""
    NX, NY = mgrid[3], mgrid[4]
    s = np.zeros((n_maps, NY, NX), np.int64)
    n = np.zeros((n_maps, NY, NX), np.int64)
    if sum_in is None:
        assert n_in is None
        return s, n
    jy, jx = np.mgrid[0:NY, 0:NX]
    for k in range(n_maps):
        sx, sy = (0, 0) if shift is None else (int(shift[k][0]), int(shift[k][1]))
        qx, qy = jx + sx, jy + sy
        ok = (qx >= 0) & (qx < NX) & (qy >= 0) & (qy < NY)
        at = (np.clip(qy, 0, NY - 1), np.clip(qx, 0, NX - 1))
        n[k] = np.clip(np.where(ok, np.asarray(n_in[k], np.int64)[at], 0), 0, n_max)
        s[k] = np.clip(np.where(ok, np.asarray(sum_in[k], np.int64)[at], 0), -n[k] * M, n[k] * M)
    return s, n


def mean_of(s, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = ((s.astype(np.float64) / n.astype(np.float64)) / 1024.0).astype(np.float32)
    mean.view(np.uint32)[n == 0] = NAN_BITS
    return mean


def fuse(height, grid, poses, mgrid, n_max, n_maps=1, sum_in=None, n_in=None, z_offset=None, map_of_frame=None, shift=None):
    """(sum_out int32, n_out int16, mean float32), each (n_maps, NY, NX), of pwpp_fuse_height_grid."""
    height = np.asarray(height, np.float32)
    frames = height.shape[0]
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    assert len(poses) in (1, frames)
    tz = np.zeros(len(poses)) if z_offset is None else np.asarray(z_offset, np.float64).reshape(-1)
    assert len(tz) == len(poses)
    if map_of_frame is None:
        assert n_maps in (1, frames)
        map_of_frame = [0] * frames if n_maps == 1 else list(range(frames))
    s, n = shifted(sum_in, n_in, mgrid, n_maps, shift, n_max)
    for f in range(frames):  # ascending: a map's frames act in this order
        k = int(map_of_frame[f])
        if k < 0:
            continue
        p = 0 if len(poses) == 1 else f
        seen, q = observe(height[f], grid, poses[p], tz[p], mgrid)
        grow = seen & (n[k] < n_max)
        cap = seen & ~grow
        share = np.sign(s[k]) * (np.abs(s[k]) // np.maximum(n[k], 1))  # truncating toward zero
        s[k] = np.where(grow, s[k] + q, np.where(cap, s[k] - share + q, s[k]))
        n[k] = np.where(grow, n[k] + 1, n[k])
        assert (np.abs(s[k]) <= n[k] * M).all()
    return s.astype(np.int32), n.astype(np.int16), mean_of(s, n)


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------
def random_heights(frames, ny, nx, seed, holes=0.3, special=True):
    """Frames of heights around -1.7 m with a share `holes` of NaN, and where they fit a few infinities, ties at x.5 / 1024, -0.0 and
    the limits +-1024 with the next float beyond."""
    rng = np.random.default_rng(seed)
    h = (rng.normal(-1.7, 0.6, (frames, ny, nx))).astype(np.float32)
    h[rng.random((frames, ny, nx)) < holes] = np.nan
    if special and h.size >= 16:
        flat = h.reshape(-1)
        beyond = np.nextafter(np.float32(1024.0), np.float32(np.inf))
        vals = np.array([np.inf, -np.inf, 0.5 / 1024, 1.5 / 1024, -2.5 / 1024, -0.0, 1024.0, -1024.0, beyond, -beyond, 1000.25, -999.75], np.float32)
        flat[rng.choice(flat.size, len(vals), replace=False)] = vals
    return h


def rigid(theta, tx, ty):
    """The pose of a rotation by theta about the origin followed by the translation (tx, ty)."""
    c, s = float(np.cos(theta)), float(np.sin(theta))
    return (c, -s, float(tx), s, c, float(ty))


def random_poses(n, seed, reach):
    rng = np.random.default_rng(seed)
    return [rigid(rng.uniform(-np.pi, np.pi), rng.uniform(-reach, reach), rng.uniform(-reach, reach)) for _ in range(n)]
