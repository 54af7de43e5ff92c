"""The contract of the correlative scan match (pwpp_match_grid, include/pwpp.h) restated in numpy double, sharing no code with the
library.  numpy on x86-64 forms no FMA and divides in IEEE, the sums are integers and the maximum has a total order, so what the
library computes must EQUAL this: no tolerance appears anywhere.

    grid  (x0, y0, cell) of the frame images, whose shape gives nx and ny          candidate  {a, b, tx, c, d, ty}, map-from-frame
    mgrid (X0, Y0, CELL, NX, NY) of the maps
"""
import numpy as np

OCCUPIED = 100
REACH = 1048576.0
BEST_DTYPE = np.dtype([("score", "<i8"), ("candidate", "<i4"), ("sx", "<i4"), ("sy", "<i4"), ("cells", "<i4")])


def landing(image, grid, candidate, mgrid):
    """(Jx, Jy) int64 arrays of the occupied cells of one frame image that land under one candidate."""
    x0, y0, cell = (np.float64(v) for v in grid)
    X0, Y0, CELL = (np.float64(v) for v in mgrid[:3])
    a, b, tx, c, d, ty = (np.float64(v) for v in candidate)
    iy, ix = np.nonzero(np.asarray(image, np.int8) == OCCUPIED)
    with np.errstate(invalid="ignore", over="ignore"):
        x = x0 + (ix.astype(np.float64) + 0.5) * cell
        y = y0 + (iy.astype(np.float64) + 0.5) * cell
        X = (a * x + b * y) + tx
        Y = (c * x + d * y) + ty
        U = (X - X0) / CELL
        V = (Y - Y0) / CELL
        lands = (U >= -REACH) & (U < REACH) & (V >= -REACH) & (V < REACH)  # (a NaN compares false)
    return np.floor(U[lands]).astype(np.int64), np.floor(V[lands]).astype(np.int64)


def scores(occupancy, grid, candidates, mgrid, maps, wx, wy, map_of_frame=None):
    """int64 (frames, n_candidates, 2 wy + 1, 2 wx + 1) of pwpp_match_grid; candidates (n_candidates, 6) or (frames, n_candidates, 6)."""
    occupancy = np.asarray(occupancy, np.int8)
    frames = occupancy.shape[0]
    maps = np.asarray(maps, np.int16)
    n_maps, NY, NX = maps.shape
    assert (NX, NY) == (mgrid[3], mgrid[4])
    cand = np.asarray(candidates, np.float64)
    cand = cand.reshape((1,) + cand.shape) if cand.ndim == 2 else cand
    assert cand.shape[0] in (1, frames) and cand.shape[2] == 6
    if map_of_frame is None:
        assert n_maps in (1, frames)
        map_of_frame = [0] * frames if n_maps == 1 else list(range(frames))
    out = np.zeros((frames, cand.shape[1], 2 * wy + 1, 2 * wx + 1), np.int64)
    for f in range(frames):
        k = int(map_of_frame[f])
        if k < 0:
            continue
        wide = maps[k].astype(np.int64)
        for r in range(cand.shape[1]):
            Jx, Jy = landing(occupancy[f], grid, cand[0 if cand.shape[0] == 1 else f, r], mgrid)
            for sy in range(-wy, wy + 1):
                qy = Jy + sy
                for sx in range(-wx, wx + 1):
                    qx = Jx + sx
                    ok = (qx >= 0) & (qx < NX) & (qy >= 0) & (qy < NY)
                    out[f, r, sy + wy, sx + wx] = wide[qy[ok], qx[ok]].sum()
    return out


def best(score, occupancy, wx, wy, map_of_frame=None):
    """The (frames,) BEST_DTYPE rows of pwpp_match_grid for the scores above."""
    occupancy = np.asarray(occupancy, np.int8)
    frames, n_candidates = score.shape[:2]
    rows = np.zeros(frames, BEST_DTYPE)
    for f in range(frames):
        rows[f]["cells"] = int((occupancy[f] == OCCUPIED).sum())
        if map_of_frame is not None and int(map_of_frame[f]) < 0:
            rows[f]["candidate"] = -1
            continue
        key = None
        for r in range(n_candidates):
            for sy in range(-wy, wy + 1):
                for sx in range(-wx, wx + 1):
                    k = (-int(score[f, r, sy + wy, sx + wx]), sx * sx + sy * sy, r, sy, sx)  # the smallest of these wins
                    if key is None or k < key:
                        key = k
        rows[f]["score"], rows[f]["candidate"], rows[f]["sy"], rows[f]["sx"] = -key[0], key[2], key[3], key[4]
    return rows


def match(occupancy, grid, candidates, mgrid, maps, wx, wy, map_of_frame=None):
    s = scores(occupancy, grid, candidates, mgrid, maps, wx, wy, map_of_frame)
    return best(s, occupancy, wx, wy, map_of_frame), s


def match_pose(candidate, CELL, sx, sy):
    a, b, tx, c, d, ty = (np.float64(v) for v in candidate)
    return np.array([a, b, tx + np.float64(sx) * np.float64(CELL), c, d, ty + np.float64(sy) * np.float64(CELL)], np.float64)
