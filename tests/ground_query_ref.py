"""The ground queries (pwpp_query_ground, pwpp_rasterize_ground) restated in numpy: czm_bins of test_gpu_point_planes.py for
the bin, the rank of the bin among the frame's patch records for the row, and the two formulas of include/pwpp.h for the
distance and the plane height.  Shared by tests/test_ground_query_cpu.py and tests/test_gpu_ground_query.py."""
import numpy as np

from test_gpu_point_planes import czm_bins

F32 = np.float32
SAMPLE_DTYPE = np.dtype([("patch", "<i4"), ("decision", "<i4"), ("ground_z", "<f4"), ("distance", "<f4")])
HIDDEN_DECISIONS = (1, 3, 5)  # not_upright, heading, tgr_reject: what PWPP_GRID_GROUND_ONLY blanks


def num_bins(p):
    return sum(a * b for a, b in zip(p.num_rings_each_zone, p.num_sectors_each_zone))


def rows_of_positions(xyz, recs, p):
    """The row of every position's bin among the patch records `recs` (-1: none), and whether numpy's bin is uncertain."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    code, near = czm_bins(xyz, p)  # (x, y only: no RNR, no FLT_MIN marker -- those are tests on cloud points)
    row_of = np.full(num_bins(p) + 1, -1, np.int64)
    row_of[recs["bin"]] = np.arange(len(recs))
    return row_of[code].astype(np.int32), near


def samples_from_rows(xyz, patch, recs):
    """The sample of every position given its row: decision, ground_z and distance from the record's normal and d."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    out = np.zeros(len(xyz), SAMPLE_DTYPE)
    out["patch"] = patch
    out["ground_z"] = np.nan
    out["distance"] = np.nan
    m = patch >= 0
    if not m.any():
        return out
    rec = recs[patch[m]]
    nrm, d = rec["normal"].astype(F32), rec["d"].astype(np.float64)
    x, y, z = (np.ascontiguousarray(xyz[m, i], F32) for i in range(3))
    with np.errstate(all="ignore"):
        # distance: calc_point_to_plane_d in float32, left to right, + d in double, one rounding (float32 arrays: no promotion)
        s = (nrm[:, 0] * x + nrm[:, 1] * y) + nrm[:, 2] * z
        dist = (s.astype(np.float64) + d).astype(F32)
        # ground_z: exact products in double, one rounding per add, one division, one rounding to float
        n0, n1, n2 = (nrm[:, i].astype(np.float64) for i in range(3))
        gz = (-((n0 * x.astype(np.float64) + n1 * y.astype(np.float64)) + d) / n2).astype(F32)
    out["decision"][m] = rec["decision"]
    out["distance"][m] = dist
    out["ground_z"][m] = gz
    return out


def restate_query(xyz, recs, p):
    """(samples, near): what pwpp_query_ground answers for `xyz` given a frame's patch records."""
    patch, near = rows_of_positions(xyz, recs, p)
    return samples_from_rows(xyz, patch, recs), near


def cell_centres(x0, y0, cell, nx, ny):
    """(ny * nx, 3) float32 centres of a grid's cells, row by row, z = 0: evaluated in double, rounded once."""
    cx = (np.float64(x0) + (np.arange(nx, dtype=np.float64) + 0.5) * np.float64(cell)).astype(F32)
    cy = (np.float64(y0) + (np.arange(ny, dtype=np.float64) + 0.5) * np.float64(cell)).astype(F32)
    out = np.zeros((ny, nx, 3), F32)
    out[..., 0] = cx[None, :]
    out[..., 1] = cy[:, None]
    return out.reshape(-1, 3)


def same_samples(a, b):
    """Bit-equal samples, NaNs compared as NaN-ness (not payload)."""
    if a.shape != b.shape or not np.array_equal(a["patch"], b["patch"]) or not np.array_equal(a["decision"], b["decision"]):
        return False
    for name in ("ground_z", "distance"):
        u, v = a[name], b[name]
        nan = np.isnan(u)
        if not np.array_equal(nan, np.isnan(v)) or not np.array_equal(u[~nan].view(np.uint32), v[~nan].view(np.uint32)):
            return False
    return True
