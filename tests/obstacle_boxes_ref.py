"""The obstacle boxes (pwpp_box_obstacles, pwpp_box_points) restated by the five steps of include/pwpp.h in numpy and Python
integers: float(int) is the correctly rounded conversion of a big integer, np.rint rounds ties to even, np.sqrt and / are IEEE,
and numpy forms no FMA.  A second, independent statement of the axis (numpy.linalg.eigh) guards against a wrong formula.  Shared
by tests/test_obstacle_boxes_cpu.py and tests/test_gpu_obstacle_boxes.py."""
import numpy as np

from obstacle_grid_ref import F32, QNAN_BITS, cells_of, height_keys, heights_of_keys

F64 = np.float64
FLOATS = ("mean_x", "mean_y", "cx", "cy", "ax", "ay", "length", "width", "sigma_long", "sigma_short", "h_min", "h_max", "z_min", "z_max")
BOX_DTYPE = np.dtype([("points", "<i4"), ("pad_", "<i4")] + [(n, "<f4") for n in FLOATS])
assert BOX_DTYPE.itemsize == 64
MAX_EXTENT = 1024.0


def moments(qx, qy):
    """Step 1's sums of one row as Python integers: N, Sx, Sy, Sxx, Sxy, Syy."""
    qx, qy = [int(v) for v in qx], [int(v) for v in qy]
    return (len(qx), sum(qx), sum(qy), sum(v * v for v in qx), sum(a * b for a, b in zip(qx, qy)), sum(v * v for v in qy))


def covariance(N, Sx, Sy, Sxx, Sxy, Syy):
    """Step 2: exact integers, each rounded once."""
    return F64(float(N * Sxx - Sx * Sx)), F64(float(N * Sxy - Sx * Sy)), F64(float(N * Syy - Sy * Sy))


def axis(a, b, c):
    """Step 3: (r, ux, uy) in double."""
    with np.errstate(all="ignore"):
        d = (a - c) * F64(0.5)
        r = np.sqrt(d * d + b * b)
        vx, vy = (d + r, b) if d >= 0 else (b, r - d)
        n = np.sqrt(vx * vx + vy * vy)
        if not (np.isfinite(n) and n > 0):
            return r, F64(1.0), F64(0.0)
        ux, uy = vx / n, vy / n
    if ux < 0 or (ux == 0 and uy < 0):
        ux, uy = -ux, -uy
    return r, ux, uy


def axis_by_eigh(a, b, c):
    """The independent statement: (unit eigenvector of the larger eigenvalue with the sign rule, eigenvalue gap relative to the
    larger eigenvalue's size)."""
    w, v = np.linalg.eigh(np.array([[a, b], [b, c]], F64))
    u = v[:, 1]
    if u[0] < 0 or (u[0] == 0 and u[1] < 0):
        u = -u
    return u, (w[1] - w[0]) / max(abs(w[1]), abs(w[0]), np.finfo(F64).tiny)


def box_rows(x0, y0, cell, nx, ny, xyz, hgt, row, max_boxes):
    """What pwpp_box_points returns: the (max_boxes,) rows of the points xyz (m, 3) float32 with heights hgt and rows row."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    hgt = np.ascontiguousarray(hgt, F32).reshape(-1)
    row = np.ascontiguousarray(row, np.int32).reshape(-1)
    x0, y0 = F64(x0), F64(y0)
    kx, _ = cells_of(xyz[:, 0], x0, cell, nx)
    ky, _ = cells_of(xyz[:, 1], y0, cell, ny)
    keep = kx & ky & ~np.isnan(hgt) & (row >= 0) & (row < max_boxes)
    out = np.zeros(max_boxes, BOX_DTYPE)
    for name in FLOATS:
        out[name] = np.uint32(QNAN_BITS).view(F32)
    dx_all = xyz[:, 0].astype(F64) - x0
    dy_all = xyz[:, 1].astype(F64) - y0
    for r in np.unique(row[keep]):
        sel = keep & (row == r)
        dx, dy = dx_all[sel], dy_all[sel]
        qx, qy = np.rint(dx * F64(1024.0)).astype(np.int64), np.rint(dy * F64(1024.0)).astype(np.int64)
        N, Sx, Sy, Sxx, Sxy, Syy = moments(qx, qy)
        a, b, c = covariance(N, Sx, Sy, Sxx, Sxy, Syy)
        rr, ux, uy = axis(a, b, c)
        o = out[r]
        o["points"] = N
        ax, ay = F32(ux), F32(uy)
        o["ax"], o["ay"] = ax, ay
        m = (a + c) * F64(0.5)
        scale = F64(N) * F64(1024.0)
        o["sigma_long"] = F32(np.sqrt(m + rr) / scale)
        o["sigma_short"] = F32(np.sqrt(max(m - rr, F64(0.0))) / scale)
        o["mean_x"] = F32(x0 + (F64(Sx) / F64(N)) / F64(1024.0))
        o["mean_y"] = F32(y0 + (F64(Sy) / F64(N)) / F64(1024.0))
        axd, ayd = F64(ax), F64(ay)
        p = (dx * axd + dy * ayd).astype(F32)
        q = (dy * axd - dx * ayd).astype(F32)
        ends = []
        for v in (p, q, hgt[sel], xyz[sel, 2]):
            k = height_keys(v)
            ends.append((heights_of_keys(np.array([k.min()], np.uint32))[0], heights_of_keys(np.array([k.max()], np.uint32))[0]))
        (pmin, pmax), (qmin, qmax) = ends[0], ends[1]
        with np.errstate(all="ignore"):
            o["length"] = F32(F64(pmax) - F64(pmin))
            o["width"] = F32(F64(qmax) - F64(qmin))
            pc = (F64(pmin) + F64(pmax)) * F64(0.5)
            qc = (F64(qmin) + F64(qmax)) * F64(0.5)
            o["cx"] = F32(x0 + (pc * axd - qc * ayd))
            o["cy"] = F32(y0 + (pc * ayd + qc * axd))
        o["h_min"], o["h_max"] = ends[2]
        o["z_min"], o["z_max"] = ends[3]
    return out


def row_moments(x0, y0, xyz):
    """(N, Sx, Sy, Sxx, Sxy, Syy) of points that all belong to one row (the tests' size assertions)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    qx = np.rint((xyz[:, 0].astype(F64) - F64(x0)) * F64(1024.0)).astype(np.int64)
    qy = np.rint((xyz[:, 1].astype(F64) - F64(y0)) * F64(1024.0)).astype(np.int64)
    return moments(qx, qy)


def rectangle(n, length, width, yaw_deg, centre, seed):
    """n points uniform in a length x width rectangle at `centre` turned by yaw_deg, z in 0..1.5: (n, 3) float32."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-length / 2, length / 2, n), rng.uniform(-width / 2, width / 2, n)
    t = np.radians(yaw_deg)
    x = centre[0] + u * np.cos(t) - v * np.sin(t)
    y = centre[1] + u * np.sin(t) + v * np.cos(t)
    return np.stack([x, y, rng.uniform(0.0, 1.5, n)], 1).astype(F32)
