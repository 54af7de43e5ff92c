"""The per-cluster map evidence of include/pwpp.h (pwpp_evidence_grid) restated in plain Python and numpy, from the header's text:
the landing in numpy float64 with one operation per statement (numpy forms no fused multiply-add), the gated read, the classes,
the rows and the verdict with dictionaries and Python integers.  Shares nothing with csrc/pwpp_evidence.h.  The GPU tests and the
stand-alone host program's dump are compared with it byte for byte."""
import numpy as np

EVIDENCE = np.dtype([("sum", "<i8"), ("cells", "<i4"), ("landed", "<i4"), ("occupied", "<i4"), ("free", "<i4"), ("unknown", "<i4"), ("verdict", "<i4")])
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
OCC_FREE, OCC_OCCUPIED, OCC_UNKNOWN = 0, 100, -1
NONE, UNDECIDED, STATIC, MOVING = -1, 0, 1, 2
CELL_NONE = -2
REACH = 1048576.0


def grid(x0, y0, cell, nx, ny):
    return dict(x0=float(x0), y0=float(y0), cell=float(cell), nx=int(nx), ny=int(ny))


def fusion_map(x0, y0, cell, nx, ny, occupied_at, free_at):
    return dict(x0=float(x0), y0=float(y0), cell=float(cell), nx=int(nx), ny=int(ny), occupied_at=int(occupied_at), free_at=int(free_at))


def rule(gate, min_cells, moving_share, static_share):
    return dict(gate=int(gate), min_cells=int(min_cells), moving_share=int(moving_share), static_share=int(static_share))


def landing(g, m, pose):
    """For every cell (iy, ix) of the grid g: (landed, Jx, Jy) in the map m under the pose; landed False where the cell does not
    land inside the map."""
    a, b, tx, c, d, ty = (np.float64(v) for v in pose)
    shape = (g["ny"], g["nx"])
    if not all(np.isfinite(v) for v in (a, b, tx, c, d, ty)):  # a pose that is not finite lands nothing
        return np.zeros(shape, bool), np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    with np.errstate(all="ignore"):
        hx = np.arange(g["nx"], dtype=np.float64) + np.float64(0.5)
        hy = np.arange(g["ny"], dtype=np.float64) + np.float64(0.5)
        sx = hx * np.float64(g["cell"])
        sy = hy * np.float64(g["cell"])
        x = np.broadcast_to(np.float64(g["x0"]) + sx, shape)
        y = np.broadcast_to((np.float64(g["y0"]) + sy)[:, None], shape)
        ax = a * x
        by = b * y
        cx = c * x
        dy = d * y
        rx = ax + by
        ry = cx + dy
        X = rx + tx
        Y = ry + ty
        nu = X - np.float64(m["x0"])
        nv = Y - np.float64(m["y0"])
        U = nu / np.float64(m["cell"])
        V = nv / np.float64(m["cell"])
        lands = (U >= -REACH) & (U < REACH) & (V >= -REACH) & (V < REACH)
        Jx = np.floor(np.where(lands, U, 0.0)).astype(np.int64)
        Jy = np.floor(np.where(lands, V, 0.0)).astype(np.int64)
        landed = lands & (Jx >= 0) & (Jx < m["nx"]) & (Jy >= 0) & (Jy < m["ny"])
    return landed, Jx, Jy


def reading(one_map, Jx, Jy, gate):
    """E of a landed cell: the maximum of the map over the gate's window inside the map."""
    NY, NX = one_map.shape
    best = None
    for ey in range(-gate, gate + 1):
        for ex in range(-gate, gate + 1):
            x, y = Jx + ex, Jy + ey
            if 0 <= x < NX and 0 <= y < NY:
                v = int(one_map[y, x])
                best = v if best is None or v > best else best
    return best


def cell_class(E, occupied_at, free_at):
    if E >= occupied_at:
        return OCC_OCCUPIED
    if E <= free_at:
        return OCC_FREE
    return OCC_UNKNOWN


def evidence_verdict(r, cells, landed, occupied, free):
    if cells == 0:
        return NONE
    if landed >= r["min_cells"] and free * 256 >= r["moving_share"] * landed:
        return MOVING
    if landed >= r["min_cells"] and occupied * 256 >= r["static_share"] * landed:
        return STATIC
    return UNDECIDED


def map_of_frame_rule(map_of_frame, n_maps, f):
    if map_of_frame is not None:
        return int(map_of_frame[f])
    return 0 if n_maps == 1 else f


def evidence_grid(g, label, occupancy_in, pose, map_of_frame, m, maps, r, max_rows):
    """pwpp_evidence_grid: label (frames, ny, nx) int32, occupancy_in the same shape int8 or None, pose (n_poses, 6), maps
    (n_maps, NY, NX) int16.  Returns (rows, cell_class, occupancy_out or None)."""
    label = np.asarray(label, np.int32)
    maps = np.asarray(maps, np.int16)
    pose = np.asarray(pose, np.float64).reshape(-1, 6)
    frames = label.shape[0]
    rows = np.zeros((frames, max_rows), EVIDENCE)
    classes = np.full(label.shape, CELL_NONE, np.int8)
    out = None if occupancy_in is None else np.array(occupancy_in, np.int8).reshape(label.shape)
    for f in range(frames):
        k = map_of_frame_rule(map_of_frame, maps.shape[0], f)
        table = {}
        if k >= 0:
            landed, Jx, Jy = landing(g, m, pose[0 if len(pose) == 1 else f])
        for iy in range(g["ny"]):
            for ix in range(g["nx"]):
                l = int(label[f, iy, ix])
                if not 0 <= l < max_rows:
                    continue
                row = table.setdefault(l, dict(sum=0, cells=0, landed=0, occupied=0, free=0, unknown=0))
                row["cells"] += 1
                if k < 0 or not landed[iy, ix]:
                    continue
                E = reading(maps[k], int(Jx[iy, ix]), int(Jy[iy, ix]), r["gate"])
                cls = cell_class(E, m["occupied_at"], m["free_at"])
                row["landed"] += 1
                row["sum"] += E
                row[{OCC_OCCUPIED: "occupied", OCC_FREE: "free", OCC_UNKNOWN: "unknown"}[cls]] += 1
                classes[f, iy, ix] = cls
        for l in range(max_rows):
            row = table.get(l, dict(sum=0, cells=0, landed=0, occupied=0, free=0, unknown=0))
            v = evidence_verdict(r, row["cells"], row["landed"], row["occupied"], row["free"])
            rows[f, l] = (row["sum"], row["cells"], row["landed"], row["occupied"], row["free"], row["unknown"], v)
        if out is not None:
            moving = np.array([rows[f, l]["verdict"] == MOVING for l in range(max_rows)])
            lab = label[f]
            named = (lab >= 0) & (lab < max_rows)
            mask = named & moving[np.where(named, lab, 0)]
            out[f][mask] = OCC_UNKNOWN
    return rows, classes, out
