"""The contract of the oriented vehicle footprint (pwpp_footprint_grid, include/pwpp.h) restated in Python, twice: `brute` asks the
coverage rule of EVERY cell of the image (and, for the cells outside it, of every cell of a box round p that plain geometry shows to hold
the rectangle) in numpy; `windowed` visits the window of Lemma 1 cell by cell in Python integers.  No GPU, no lanes, no slots.

`certify` checks given rows against the brute force and returns what differs."""
import math

import numpy as np

import reach_ref as rr

FREE, HIT, SKIPPED = 0, 1, 2
OUTSIDE_BLOCKS = 1
SUB, MAX_EXTENT, MAX_STEPS = 16, 1024, 4096
BEYOND, REACH_NONE = rr.DIST_BEYOND, rr.NONE
POSE_ROW = np.dtype([(n, "<i4") for n in ("status", "covered", "outside", "blocked", "unknown", "max_term", "min_dist2", "hit")])
TRAJ_ROW = np.dtype([(n, "<i4") for n in ("first_hit", "free_steps", "last", "max_term", "sum_term", "unknown", "min_dist2", "reach_last")])
SKIPPED_ROW = (SKIPPED, 0, 0, 0, 0, 0, BEYOND, -1)
FAR = 1536  # ticks: a covered centre is a point of the rectangle, at most sqrt(2) * 1024 < 1449 from p; a centre farther along an axis is never covered


def foot_params(front=0, rear=0, half_width=0, flags=0):
    return dict(front=front, rear=rear, half_width=half_width, flags=flags)


def covers(fp, pose, ix, iy):
    """The rule, in Python integers, for any cell."""
    px, py, ux, uy = (int(v) for v in pose)
    if ux == 0 and uy == 0:
        return False
    dx, dy = 16 * int(ix) + 8 - px, 16 * int(iy) + 8 - py
    a, b, n2 = ux * dx + uy * dy, ux * dy - uy * dx, ux * ux + uy * uy
    along = fp["front"] if a >= 0 else fp["rear"]
    return a * a <= along * along * n2 and b * b <= fp["half_width"] ** 2 * n2


def covered_mask(fp, pose, xs, ys):
    """The rule for the cells ys x xs (int64 arrays of indices) as a boolean (len(ys), len(xs)) array."""
    px, py, ux, uy = (int(v) for v in pose)
    dx = np.clip(16 * np.asarray(xs, np.int64) + 8 - px, -FAR, FAR)[None, :]  # (a clipped cell stays beyond the diagonal: never covered)
    dy = np.clip(16 * np.asarray(ys, np.int64) + 8 - py, -FAR, FAR)[:, None]
    a, b, n2 = ux * dx + uy * dy, ux * dy - uy * dx, ux * ux + uy * uy
    along = np.where(a >= 0, fp["front"], fp["rear"]).astype(np.int64)
    return (a * a <= along * along * n2) & (b * b <= fp["half_width"] ** 2 * n2)


def _row(fp, covered, outside, t, cost, d2, idx):
    """The pose row from the covered cells inside the image: their terms, cost bytes, dist2 (or None) and indices."""
    blocked = t == 0
    hit = blocked.any() or (outside > 0 and fp["flags"] & OUTSIDE_BLOCKS)
    return (HIT if hit else FREE, covered, outside, int(blocked.sum()), int((cost < 0).sum()), int(t.max()) if t.size else 0,
            int(d2.min()) if d2 is not None and d2.size else BEYOND, int(idx[blocked].min()) if blocked.any() else -1)


def pose_row_brute(t, cost, dist2, fp, pose):
    """One pose on one frame; t: rr.terms_array(cost, None, p, dist2)."""
    if pose[2] == 0 and pose[3] == 0:
        return SKIPPED_ROW
    ny, nx = cost.shape
    m = covered_mask(fp, pose, np.arange(nx), np.arange(ny))
    cx, cy = int(pose[0]) >> 4, int(pose[1]) >> 4
    r = (math.isqrt(max(fp["front"], fp["rear"]) ** 2 + fp["half_width"] ** 2) + 1) // 16 + 2  # cells: the rectangle's diagonal from p, and a margin
    bx, by = np.arange(cx - r, cx + r + 1), np.arange(cy - r, cy + r + 1)
    box = covered_mask(fp, pose, bx, by)
    inside_box = ((by >= 0) & (by < ny))[:, None] & ((bx >= 0) & (bx < nx))[None, :]
    outside = int((box & ~inside_box).sum())
    idx = np.arange(nx * ny).reshape(ny, nx)
    return _row(fp, int(m.sum()) + outside, outside, t[m], cost[m], None if dist2 is None else dist2[m], idx[m])


def window(fp, pose):
    """(x0, y0, w, h) of the window csrc/pwpp_footprint.h visits: the cells whose centres lie in the rectangle's bounding box round p, by
    the support S / n along each axis rounded up; the E + W square of Lemma 1 where that has at most 5 cells a side."""
    px, py, ux, uy = (int(v) for v in pose)
    f, r, hw = fp["front"], fp["rear"], fp["half_width"]
    both = max(f, r) + hw
    xm = xp = ym = yp = both
    if 2 * both // 16 + 1 > 5:
        n2 = ux * ux + uy * uy

        def over_norm(S):  # ceil(S / sqrt(n2))
            m = math.isqrt(S * S // n2)
            while m * m * n2 < S * S:
                m += 1
            return m

        xp, xm = over_norm(max(f * ux, -r * ux) + hw * abs(uy)), over_norm(max(-f * ux, r * ux) + hw * abs(uy))
        yp, ym = over_norm(max(f * uy, -r * uy) + hw * abs(ux)), over_norm(max(-f * uy, r * uy) + hw * abs(ux))
    x0, y0 = -((-(px - xm - 8)) // 16), -((-(py - ym - 8)) // 16)  # ceil
    return x0, y0, (px + xp - 8) // 16 - x0 + 1, (py + yp - 8) // 16 - y0 + 1


def pose_row_windowed(t, cost, dist2, fp, pose):
    if pose[2] == 0 and pose[3] == 0:
        return SKIPPED_ROW
    ny, nx = cost.shape
    x0, y0, w, h = window(fp, pose)
    covered = outside = blocked = unknown = max_term = 0
    min_d2, hit = BEYOND, -1
    for iy in range(y0, y0 + h):
        for ix in range(x0, x0 + w):
            if not covers(fp, pose, ix, iy):
                continue
            covered += 1
            if not (0 <= ix < nx and 0 <= iy < ny):
                outside += 1
                continue
            unknown += int(cost[iy, ix]) < 0
            max_term = max(max_term, int(t[iy, ix]))
            if dist2 is not None:
                min_d2 = min(min_d2, int(dist2[iy, ix]))
            if t[iy, ix] == 0:
                blocked += 1
                hit = iy * nx + ix if hit < 0 else hit  # (rows ascending, columns ascending: the first is the smallest)
    status = HIT if blocked or (outside and fp["flags"] & OUTSIDE_BLOCKS) else FREE
    return (status, covered, outside, blocked, unknown, max_term, min_d2, hit)


def traj_row(rows, poses, reach, nx, ny):
    """The trajectory row of one trajectory: rows (n_steps,) POSE_ROW, poses (n_steps, 4), reach (ny, nx) or None."""
    hits = np.flatnonzero(rows["status"] == HIT)
    first = int(hits[0]) if hits.size else -1
    k = np.arange(len(rows))
    free = (rows["status"] != SKIPPED) & ((k < first) if first >= 0 else True)
    last = int(k[free].max()) if free.any() else -1
    rl = REACH_NONE
    if reach is not None and last >= 0:
        cx, cy = int(poses[last][0]) >> 4, int(poses[last][1]) >> 4
        if 0 <= cx < nx and 0 <= cy < ny:
            rl = int(reach[cy, cx])
    f = rows[free]
    return (first, int(free.sum()), last, int(f["max_term"].max()) if f.size else 0, int(f["max_term"].sum()), int(f["unknown"].sum()),
            int(f["min_dist2"].min()) if f.size else BEYOND, rl)


def as_frames(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a.reshape((1,) + a.shape) if a.ndim == 2 else a


def as_poses(poses):
    """(n_sets, n_traj, n_steps, 4) from that, (n_traj, n_steps, 4) or (n_steps, 4)."""
    q = np.ascontiguousarray(poses, np.int32)
    while q.ndim < 4:
        q = q.reshape((1,) + q.shape)
    assert q.ndim == 4 and q.shape[-1] == 4
    return q


def footprints(cost, p, fp, poses, dist2=None, reach=None, method="brute"):
    """(pose_rows (frames, n_traj, n_steps), traj_rows (frames, n_traj)) of the contract; p: rr.params, fp: foot_params."""
    c3 = as_frames(cost, np.int8)
    d3 = None if dist2 is None else as_frames(dist2, np.int32).reshape(c3.shape)
    r3 = None if reach is None else as_frames(reach, np.int32).reshape(c3.shape)
    q = as_poses(poses)
    frames, ny, nx = c3.shape
    sets, n_traj, n_steps = q.shape[:3]
    assert sets in (1, frames)
    one = pose_row_brute if method == "brute" else pose_row_windowed
    prow, trow = np.zeros((frames, n_traj, n_steps), POSE_ROW), np.zeros((frames, n_traj), TRAJ_ROW)
    for f in range(frames):
        t = rr.terms_array(c3[f], None, p, None if d3 is None else d3[f])
        qs = q[f if sets > 1 else 0]
        memo = {}  # (a fan repeats poses)
        for j in range(n_traj):
            for k in range(n_steps):
                key = qs[j, k].tobytes()
                if key not in memo:
                    memo[key] = one(t, c3[f], None if d3 is None else d3[f], fp, qs[j, k])
                prow[f, j, k] = memo[key]
            trow[f, j] = traj_row(prow[f, j], qs[j], None if r3 is None else r3[f], nx, ny)
    return prow, trow


def certify(cost, p, fp, poses, pose_rows=None, traj_rows=None, dist2=None, reach=None):
    """What of the given rows differs from the brute force: a list of strings, empty where they are the contract's."""
    wp, wt = footprints(cost, p, fp, poses, dist2, reach, "brute")
    bad = []
    for name, got, want in (("pose", pose_rows, wp), ("trajectory", traj_rows, wt)):
        if got is None:
            continue
        got = np.asarray(got).reshape(want.shape)
        for at in zip(*np.nonzero(got != want)):
            bad.append("%s row %s: %s, the contract has %s" % (name, at, got[at], want[at]))
    return bad


def touches(fp, pose, ix, iy):
    """Whether the exact rectangle and the closed square of cell (ix, iy) share a point, in integers: two convex polygons are disjoint
    iff one of their edge normals separates them -- the axes x, y, u and u' here.  Everything is scaled by n2 where u is used."""
    px, py, ux, uy = (int(v) for v in pose)
    if ux == 0 and uy == 0:
        return False
    n2 = ux * ux + uy * uy
    corners = [(16 * ix + cx - px, 16 * iy + cy - py) for cx in (0, 16) for cy in (0, 16)]
    # along u and across it: the square's extent against the rectangle's, both times sqrt(n2): compare squares with signs
    al = [ux * x + uy * y for x, y in corners]
    ac = [ux * y - uy * x for x, y in corners]

    def beyond(v, limit):  # v / sqrt(n2) > limit, limit >= 0
        return v > 0 and v * v > limit * limit * n2

    if beyond(min(al), fp["front"]) or beyond(-max(al), fp["rear"]) or beyond(min(ac), fp["half_width"]) or beyond(-max(ac), fp["half_width"]):
        return False
    # along x and y: the rectangle's extent in the direction c in {(+-1, 0), (0, +-1)}, times sqrt(n2), is the exact integer
    # max(front (c . u), -rear (c . u)) + half_width |c . u'|, never negative (the rectangle holds p)
    def support(cx, cy):
        s, w = cx * ux + cy * uy, -cx * uy + cy * ux
        return max(fp["front"] * s, -fp["rear"] * s) + fp["half_width"] * abs(w)

    xs, ys = [c[0] for c in corners], [c[1] for c in corners]
    for lo, sup in ((min(xs), support(1, 0)), (-max(xs), support(-1, 0)), (min(ys), support(0, 1)), (-max(ys), support(0, -1))):
        if lo > 0 and lo * lo * n2 > sup * sup:
            return False
    return True


def random_images(frames, ny, nx, seed, walls=3):
    """Cost images with walls and unknown cells: mostly cheap ground, a few lethal bars, a share of unknown."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 40, (frames, ny, nx)).astype(np.int8)
    for f in range(frames):
        for _ in range(walls):
            if rng.random() < 0.5:
                y, x0, x1 = rng.integers(0, ny), *sorted(rng.integers(0, nx + 1, 2))
                c[f, y, x0:x1] = 100
            else:
                x, y0, y1 = rng.integers(0, nx), *sorted(rng.integers(0, ny + 1, 2))
                c[f, y0:y1, x] = 110
    u = rng.random((frames, ny, nx))
    c[u > 0.93] = -1
    return c
