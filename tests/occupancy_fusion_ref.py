"""The contract of the occupancy fusion (pwpp_fuse_grid, include/pwpp.h) restated in numpy double: vectorised over the map's cells,
looping over the frames in order, sharing no code with the library.  numpy on x86-64 forms no FMA and divides in IEEE, so what
the library computes must EQUAL this: no tolerance appears anywhere.

    grid  (x0, y0, cell) of the frame images, whose shape gives nx and ny          pose  {a, b, tx, c, d, ty}, map-from-frame
    mgrid (X0, Y0, CELL, NX, NY) of the maps                                         par   (hit, miss, l_min, l_max, occupied_at, free_at)
"""
import numpy as np

FREE, OCCUPIED, UNKNOWN = 0, 100, -1
QUADRANTS = (0.25, 0.75)  # 0.25 + 0.5 * q
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
PAR = (40, 20, -200, 350, 60, -40)  # the parameters most tests use


def sample(image, grid, pose, mx, my):
    """The bytes the positions (mx, my) of the map's frame read in one frame image."""
    x0, y0, cell = grid
    ny, nx = image.shape
    a, b, tx, c, d, ty = (np.float64(v) for v in pose)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = mx - tx
        dy = my - ty
        fx = a * dx + c * dy
        fy = b * dx + d * dy
        u = (fx - np.float64(x0)) / np.float64(cell)
        v = (fy - np.float64(y0)) / np.float64(cell)
        inside = (u >= 0) & (u < nx) & (v >= 0) & (v < ny)  # (a NaN compares false)
    ix = np.where(inside, np.floor(np.where(inside, u, 0.0)), 0).astype(np.int64)
    iy = np.where(inside, np.floor(np.where(inside, v, 0.0)), 0).astype(np.int64)
    return np.where(inside, image[iy, ix], UNKNOWN)


def observe(image, grid, pose, mgrid, offsets=QUADRANTS):
    """(occupied, free) of every map cell in one frame; offsets (0.5,) is the centre sampling the contract rejects."""
    X0, Y0, CELL, NX, NY = mgrid
    jy, jx = np.mgrid[0:NY, 0:NX]
    occupied = np.zeros((NY, NX), bool)
    free = np.ones((NY, NX), bool)
    for oy in offsets:
        my = np.float64(Y0) + (jy.astype(np.float64) + oy) * np.float64(CELL)
        for ox in offsets:
            mx = np.float64(X0) + (jx.astype(np.float64) + ox) * np.float64(CELL)
            s = sample(image, grid, pose, mx, my)
            occupied |= s == OCCUPIED
            free &= s == FREE
    return occupied, free & ~occupied


def shifted(map_in, mgrid, n_maps, shift):
    NX, NY = mgrid[3], mgrid[4]
    out = np.zeros((n_maps, NY, NX), np.int64)
    if map_in is None:
        return out
    jy, jx = np.mgrid[0:NY, 0:NX]
    for k in range(n_maps):
        sx, sy = (0, 0) if shift is None else (int(shift[k][0]), int(shift[k][1]))
        qx, qy = jx + sx, jy + sy
        ok = (qx >= 0) & (qx < NX) & (qy >= 0) & (qy < NY)
        out[k] = np.where(ok, np.asarray(map_in[k], np.int64)[np.clip(qy, 0, NY - 1), np.clip(qx, 0, NX - 1)], 0)
    return out


def byte_of(L, par):
    return np.where(L >= par[4], OCCUPIED, np.where(L <= par[5], FREE, UNKNOWN)).astype(np.int8)


def fuse(occupancy, grid, poses, mgrid, par=PAR, n_maps=1, map_in=None, map_of_frame=None, shift=None, offsets=QUADRANTS):
    """(map_out int16 (n_maps, NY, NX), map_occupancy int8) of pwpp_fuse_grid."""
    occupancy = np.asarray(occupancy, np.int8)
    frames = occupancy.shape[0]
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    assert len(poses) in (1, frames)
    if map_of_frame is None:
        assert n_maps in (1, frames)
        map_of_frame = [0] * frames if n_maps == 1 else list(range(frames))
    hit, miss, l_min, l_max = par[:4]
    L = shifted(map_in, mgrid, n_maps, shift)
    for f in range(frames):  # ascending: a map's frames act in this order
        k = int(map_of_frame[f])
        if k < 0:
            continue
        occupied, free = observe(occupancy[f], grid, poses[0 if len(poses) == 1 else f], mgrid, offsets)
        L[k] = np.where(occupied, np.minimum(L[k] + hit, l_max), np.where(free, np.maximum(L[k] - miss, l_min), L[k]))
    assert L.min() >= -32768 and L.max() <= 32767
    return L.astype(np.int16), byte_of(L, par)


# ---- inputs the tests share ------------------------------------------------------------------------------------------------------
def random_occupancy(frames, ny, nx, seed, p=(0.55, 0.15, 0.3), stray=True):
    """Frames of the three bytes with the shares p = (free, occupied, unknown), and a few stray bytes 50."""
    rng = np.random.default_rng(seed)
    occ = rng.choice(np.array([FREE, OCCUPIED, UNKNOWN], np.int8), size=(frames, ny, nx), p=p)
    if stray and occ.size >= 4:
        occ.reshape(-1)[rng.integers(0, occ.size, max(1, occ.size // 50))] = 50
    return occ


def rigid(theta, tx, ty):
    """The pose of a rotation by theta about the origin followed by the translation (tx, ty)."""
    c, s = float(np.cos(theta)), float(np.sin(theta))
    return (c, -s, float(tx), s, c, float(ty))


def random_poses(n, seed, reach):
    rng = np.random.default_rng(seed)
    return [rigid(rng.uniform(-np.pi, np.pi), rng.uniform(-reach, reach), rng.uniform(-reach, reach)) for _ in range(n)]
