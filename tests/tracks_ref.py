"""The cluster association of include/pwpp.h (pwpp_associate_grid) restated in plain Python and numpy, from the header's text: the
geometry in numpy float64 with one operation per statement (numpy forms no fused multiply-add), the votes, overlaps, links and
ids with dictionaries and Python integers.  Shares nothing with csrc/pwpp_tracks.h.  The GPU tests and the stand-alone host
program's dump are compared with it byte for byte."""
import numpy as np

LINK = np.dtype([("other", "<i4"), ("overlap", "<i4"), ("cells", "<i4"), ("links", "<i4")])
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def grid(x0, y0, cell, nx, ny):
    return dict(x0=float(x0), y0=float(y0), cell=float(cell), nx=int(nx), ny=int(ny))


def previous_cells(gc, gp, pose):
    """For every current cell (jy, jx): (has, px, py), the previous cell under its centre; has False where there is none."""
    a, b, tx, c, d, ty = (np.float64(v) for v in pose)
    with np.errstate(all="ignore"):
        jx = np.arange(gc["nx"], dtype=np.float64)
        jy = np.arange(gc["ny"], dtype=np.float64)
        hx = jx + np.float64(0.5)
        hy = jy + np.float64(0.5)
        sx = hx * np.float64(gc["cell"])
        sy = hy * np.float64(gc["cell"])
        mx = np.float64(gc["x0"]) + sx
        my = np.float64(gc["y0"]) + sy
        dx = np.broadcast_to(mx - tx, (gc["ny"], gc["nx"]))
        dy = np.broadcast_to((my - ty)[:, None], (gc["ny"], gc["nx"]))
        adx = a * dx
        cdy = c * dy
        fx = adx + cdy
        bdx = b * dx
        ddy = d * dy
        fy = bdx + ddy
        nu = fx - np.float64(gp["x0"])
        nv = fy - np.float64(gp["y0"])
        u = nu / np.float64(gp["cell"])
        v = nv / np.float64(gp["cell"])
        has = (u >= 0.0) & (u < float(gp["nx"])) & (v >= 0.0) & (v < float(gp["ny"]))
        px = np.where(has, np.floor(np.where(has, u, 0.0)), 0.0).astype(np.int64)
        py = np.where(has, np.floor(np.where(has, v, 0.0)), 0.0).astype(np.int64)
    return has, px, py


def vote(prev, px, py, gate, max_rows):
    """The row the current cell with previous cell (px, py) votes for, or -1."""
    nyp, nxp = prev.shape
    best = None
    for ey in range(-gate, gate + 1):
        for ex in range(-gate, gate + 1):
            x, y = px + ex, py + ey
            if not (0 <= x < nxp and 0 <= y < nyp):
                continue
            l = int(prev[y, x])
            if not 0 <= l < max_rows:
                continue
            key = (ex * ex + ey * ey, y * nxp + x)
            if best is None or key < best[0]:
                best = (key, l)
    return -1 if best is None else best[1]


def pair_counts(curr, prev, gc, gp, pose, gate, max_rows):
    """{(a, b): n(a, b)} of one frame pair."""
    has, px, py = previous_cells(gc, gp, pose)
    n = {}
    for jy, jx in zip(*np.nonzero((curr >= 0) & (curr < max_rows) & has)):
        a = vote(prev, int(px[jy, jx]), int(py[jy, jx]), gate, max_rows)
        if a >= 0:
            key = (a, int(curr[jy, jx]))
            n[key] = n.get(key, 0) + 1
    return n


def associate(curr, prev, gc, gp, poses, gate, min_overlap, max_rows, max_pairs, id_prev=None, next_id=None):
    """curr (frames, gc.ny, gc.nx) and prev (frames, gp.ny, gp.nx) int32; poses (1, 6) or (frames, 6).  Returns a dictionary of
    curr_links, prev_links (frames, max_rows) of LINK, n_pairs (frames,), and with ids id_curr (frames, max_rows), next_id_out."""
    curr, prev = np.asarray(curr, np.int32), np.asarray(prev, np.int32)
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    frames = curr.shape[0]
    cl, pl = np.zeros((frames, max_rows), LINK), np.zeros((frames, max_rows), LINK)
    n_pairs = np.zeros(frames, np.int32)
    with_ids = id_prev is not None
    id_curr = np.full((frames, max_rows), -1, np.int32) if with_ids else None
    next_out = np.zeros(frames, np.int32) if with_ids else None
    for f in range(frames):
        n = pair_counts(curr[f], prev[f], gc, gp, poses[0 if len(poses) == 1 else f], gate, max_rows)
        over = len(n) > max_pairs
        n_pairs[f] = max_pairs + 1 if over else len(n)
        for table, image, side in ((cl, curr[f], 1), (pl, prev[f], 0)):
            partners = {}
            for k, v in n.items():
                partners.setdefault(k[side], {})[k[1 - side]] = v
            named = image[(image >= 0) & (image < max_rows)]
            count = np.bincount(named, minlength=max_rows)
            for r in range(max_rows):
                cells = int(count[r])
                mine = partners.get(r, {})
                if over:
                    table[f, r] = (-2, 0, cells, 0)
                elif not mine:
                    table[f, r] = (-1, 0, cells, 0)
                else:
                    most = max(mine.values())
                    other = min(k for k, v in mine.items() if v == most)
                    table[f, r] = (other, most, cells, len(mine))
        if with_ids:
            fresh, first = 0, int(next_id[f])
            for b in range(max_rows):
                if cl[f, b]["cells"] <= 0:
                    continue
                a = int(cl[f, b]["other"])
                if a >= 0 and int(pl[f, a]["other"]) == b and int(cl[f, b]["overlap"]) >= min_overlap and int(id_prev[f][a]) >= 0:
                    id_curr[f, b] = int(id_prev[f][a])
                else:
                    id_curr[f, b] = (first + fresh) & 0x7FFFFFFF
                    fresh += 1
            next_out[f] = (first + fresh) & 0x7FFFFFFF
    out = dict(curr_links=cl, prev_links=pl, n_pairs=n_pairs)
    if with_ids:
        out.update(id_curr=id_curr, next_id_out=next_out)
    return out


def blobs(frames, ny, nx, seed, n_blobs=6, max_rows=8):
    """Random label images: rectangles of labels -1 .. max_rows + 1 painted over an unlabelled ground, later ones on top."""
    rng = np.random.default_rng(seed)
    out = np.full((frames, ny, nx), -1, np.int32)
    for f in range(frames):
        for _ in range(n_blobs):
            x, y = int(rng.integers(0, nx)), int(rng.integers(0, ny))
            w, h = int(rng.integers(1, max(2, nx // 2 + 1))), int(rng.integers(1, max(2, ny // 2 + 1)))
            out[f, y:y + h, x:x + w] = int(rng.integers(0, max_rows))
    return out


def yaw(deg, tx=0.0, ty=0.0):
    """The pose of a rotation by deg degrees (a quarter turn exactly for multiples of 90) and a shift."""
    q = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}.get(deg % 360)
    co, si = q if q else (float(np.cos(np.radians(deg))), float(np.sin(np.radians(deg))))
    return (co, -si, float(tx), si, co, float(ty))
