"""The contract of the terrain analysis (pwpp_terrain_grid, include/pwpp.h) restated in numpy integers and double, sharing no code
with the library: the moments are int64 sums over the (2r+1)^2 shifted copies of the quantised image, N is computed in Python
integers (object arrays) and converted by float(int), which rounds once to nearest even, sqrt and / are numpy's, correctly rounded.
No tolerance anywhere: the tests compare bits, and a NaN is 0x7fc00000."""
import numpy as np

NAN_BITS = 0x7FC00000
M = 1 << 20
INF = float("inf")
NAMES = ("step", "slope", "rough", "count", "cost")


def quantise(height):
    """(known, z): where a float32 height image has a known cell, and its height in units of 2^-10 m (int64, 0 where unknown)."""
    z = np.asarray(height, np.float32).astype(np.float64)
    known = np.isfinite(z) & (np.abs(z) <= 1024.0)
    return known, np.rint(np.where(known, z, 0.0) * 1024.0).astype(np.int64)


def moments(height, radius):
    """The window sums of every cell of a (frames, ny, nx) image as a dict of int64 arrays, with zmin, zmax (0 where k == 0)."""
    known, z = quantise(height)
    f, ny, nx = z.shape
    r = int(radius)
    kp = np.zeros((f, ny + 2 * r, nx + 2 * r), np.int64)
    zp = np.zeros_like(kp)
    kp[:, r:r + ny, r:r + nx], zp[:, r:r + ny, r:r + nx] = known, z
    S = {n: np.zeros((f, ny, nx), np.int64) for n in ("k", "x", "y", "z", "xx", "xy", "yy", "xz", "yz", "zz")}
    zmin, zmax = np.full((f, ny, nx), 2 * M, np.int64), np.full((f, ny, nx), -2 * M, np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            kk = kp[:, r + dy:r + dy + ny, r + dx:r + dx + nx]
            zz = zp[:, r + dy:r + dy + ny, r + dx:r + dx + nx]   # (0 where unknown)
            S["k"] += kk
            S["x"] += dx * kk
            S["y"] += dy * kk
            S["xx"] += dx * dx * kk
            S["xy"] += dx * dy * kk
            S["yy"] += dy * dy * kk
            S["z"] += zz
            S["xz"] += dx * zz
            S["yz"] += dy * zz
            S["zz"] += zz * zz
            zmin = np.where(kk == 1, np.minimum(zmin, zz), zmin)
            zmax = np.where(kk == 1, np.maximum(zmax, zz), zmax)
    S["zmin"], S["zmax"] = np.where(S["k"] > 0, zmin, 0), np.where(S["k"] > 0, zmax, 0)
    S["known"] = known
    return S


def plane(S):
    """(D, A, B) as int64 arrays and N as an object array of Python integers."""
    k = S["k"]
    C = lambda u, v, uv: k * S[uv] - S[u] * S[v]
    Cxx, Cxy, Cyy, Cxz, Cyz, Czz = C("x", "x", "xx"), C("x", "y", "xy"), C("y", "y", "yy"), C("x", "z", "xz"), C("y", "z", "yz"), C("z", "z", "zz")
    D, A, B = Cxx * Cyy - Cxy * Cxy, Cxz * Cyy - Cyz * Cxy, Cyz * Cxx - Cxz * Cxy
    O = lambda a: a.astype(object)
    N = O(D) * O(Czz) - O(A) * O(Cxz) - O(B) * O(Cyz)
    return D, A, B, N


def _set_nan(img, where):
    img.view(np.uint32)[where] = NAN_BITS


def terrain(height, cell, radius=1, min_known=3, step_max=INF, slope_max=INF, rough_max=INF):
    """(step, slope, rough float32, count uint8, cost int8) of pwpp_terrain_grid, each in the shape of `height`:
    (frames, ny, nx) or (ny, nx)."""
    h = np.asarray(height, np.float32)
    h3 = h.reshape((1,) + h.shape) if h.ndim == 2 else h
    S = moments(h3, radius)
    D, A, B, N = plane(S)
    k, known = S["k"], S["known"]
    flat = D != 0
    with np.errstate(all="ignore"):
        step = ((S["zmax"] - S["zmin"]).astype(np.float64) / 1024.0).astype(np.float32)
        a, b, d = A.astype(np.float64), B.astype(np.float64), np.where(flat, D, 1).astype(np.float64)
        slope = (np.sqrt(a * a + b * b) / (d * (1024.0 * float(cell)))).astype(np.float32)
        Nd = np.array([float(v) for v in N.ravel()], np.float64).reshape(N.shape)
        rough = (np.sqrt(Nd / (d * (k * k).astype(np.float64))) / 1024.0).astype(np.float32)
        t = np.zeros(k.shape, np.float64)
        for v, lim in ((step, step_max), (slope, slope_max), (rough, rough_max)):
            lim = np.float32(lim)
            if not np.isinf(lim):
                t = np.maximum(t, v.astype(np.float64) / np.float64(lim))
        cost = np.where(t >= 1.0, 100.0, np.floor(t * 100.0))
    cost = np.where(known & flat & (k >= int(min_known)), cost, -1.0).astype(np.int8)
    _set_nan(step, ~known)
    _set_nan(slope, ~(known & flat))
    _set_nan(rough, ~(known & flat))
    return tuple(o.reshape(h.shape) for o in (step, slope, rough, k.astype(np.uint8), cost))


def same(a, b):
    """Whether two tuples of outputs hold the same bytes (None: an output that was not asked for matches anything)."""
    return all(x is None or y is None or (x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def random_heights(frames, ny, nx, seed, holes=0.3, limits=False):
    """A rolling surface with noise, `holes` of it NaN; limits: also heights of +-1024 and just beyond, infinities, -0.0 and ties."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    h = np.empty((frames, ny, nx), np.float32)
    for f in range(frames):
        h[f] = 0.3 * np.sin(0.4 * xx + f) + 0.05 * yy - 0.02 * xx + rng.normal(0.0, 0.03, (ny, nx)) + rng.uniform(-2, 2)
    if limits:
        beyond = np.nextafter(np.float32(1024.0), np.float32(np.inf))
        special = np.array([1024.0, -1024.0, beyond, -beyond, INF, -INF, -0.0, 0.5 / 1024, 1.5 / 1024, -2.5 / 1024, 1023.9, -1023.9], np.float32)
        pick = rng.random((frames, ny, nx)) < 0.15
        h[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    h[rng.random((frames, ny, nx)) < holes] = np.nan
    return h
