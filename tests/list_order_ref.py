"""The order PWPP_ORDER_REFERENCE promises inside every part of the index lists, restated, and clouds whose parts have chosen
lengths and heights (TEST INFRASTRUCTURE, numpy only).

THE CONTRACT (include/pwpp.h at PWPP_ORDER_REFERENCE): ground candidates ascending in z; non-ground points grouped by the R-VPF
round that removed them, then the rest, each group ascending in z; small bins, RNR hits and out-of-range points in cloud order;
equal z -- and -0.0 == +0.0 -- in cloud order.  `expected_lists` applies exactly that to the oracle's lists, whose parts and
categories the restatement exports (oracle_ext.h, pwo_ext_get_list_keys); the oracle's own order among equal heights is libstdc++'s.

THE CLOUDS put L points with chosen heights into one bin of the CZM (limits from the parameters) and surround them so that the
bin behaves as wanted: a floor within +-0.03 m of -sensor_height is a ground part of exactly L entries; a narrow column over a
floor of 64 points is a non-ground part (category 255) of exactly L; points beyond max_range or inside min_range are a
pseudo-bin of L; nine points are a small bin.  Rows are shuffled with a fixed seed: ties are interleaved in cloud index.

`sort_path` restates which path K7 (k_order_sublists, pwpp_kernels.hip) takes for a part of one tile -- for the ACCOUNT of what
the cases reach (test_list_order_cpu.py, profiles/list_order_cases.txt), never for an expected value.
"""
import math

import numpy as np

import oracle_lib as ol

WAVE_MAX = 256        # the wave instantiation's longest list
TILE = 4096           # kOrdTile of the workgroup instantiation
BUCKET_TILE = 4032    # kBucketTile: the longest tile the distribution sort is offered
BUCKETS = 1024        # kOrdBuckets
MAX_BUCKET = 32       # kOrdMaxBucket
SENSOR_HEIGHT = 1.723
FLOOR_POINTS = 64     # the floor under a column


# ---------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------
def canonical(z):
    """z with -0.0 taken as +0.0 (the comparator a.z < b.z holds them equal)."""
    z = np.array(z, np.float32)
    z[z == 0.0] = 0.0
    return z


def _expected(z, idx, part, cat, part_cloud):
    idx = np.asarray(idx, np.int64)
    part = np.asarray(part, np.int64)
    cloud = np.asarray(part_cloud, bool)[part] if len(part) else np.zeros(0, bool)
    assert np.array_equal(part, np.sort(part)), "parts are contiguous and numbered in list order"
    assert not np.asarray(cat)[cloud].any(), "a part in cloud order has category 0 throughout"
    zc = canonical(z[idx])
    zc[cloud] = 0.0
    assert not np.isnan(zc).any()  # (NaN heights: undefined by the header)
    order = np.lexsort((idx, zc, np.asarray(cat, np.int64), part))  # last key first: part, category, height, cloud index
    out = idx[order]
    # what was taken: an order among equal heights, nothing else
    mine = np.stack([part, np.asarray(cat, np.int64)[order], out], axis=1)
    theirs = np.stack([part, np.asarray(cat, np.int64), idx], axis=1)
    assert np.array_equal(mine[np.lexsort(mine.T[::-1])], theirs[np.lexsort(theirs.T[::-1])]), "per (part, category) the same indices"
    keep = ~cloud
    assert np.array_equal(z[out][keep], z[idx][keep]), "the z sequence (under ==) is the oracle's"
    assert np.array_equal(np.asarray(cat)[order][keep], np.asarray(cat)[keep])
    return out.astype(np.int32)


def expected_lists(pts, result):
    """(ground, nonground) index lists the contract demands for the frame `pts`, from an oracle_lib.Result of the restatement."""
    z = np.ascontiguousarray(pts[:, 2], np.float32)
    return (_expected(z, result.ground_idx, result.ground_part, result.ground_cat, result.ground_part_cloud),
            _expected(z, result.nonground_idx, result.nonground_part, result.nonground_cat, result.nonground_part_cloud))


# ---------------------------------------------------------------------------------------------------------------
# which path K7 takes
# ---------------------------------------------------------------------------------------------------------------
def fullest_bucket(z):
    """ord_bucket_sort's bucket of every height, in its own float32 chain: subtract, multiply by 1024 / range, truncate, clamp.
    Returns (largest count, scale); the count is None where the scale is not finite and positive."""
    z = canonical(z)
    z0 = z.min()
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        rng = np.float32(z.max() - z0)
        scale = np.float32(np.float32(BUCKETS) / rng)
        if not (scale <= np.finfo(np.float32).max) or not (scale > 0):
            return None, scale
        v = ((z - z0).astype(np.float32) * scale).astype(np.float32)
    b = np.clip(np.trunc(v.astype(np.float64)), 0, BUCKETS - 1).astype(np.int64)
    return int(np.bincount(b, minlength=BUCKETS).max()), scale


def sort_path(cat, z, cloud_order=False):
    """'wave', 'bucket' or 'network:<reason>' for a part of at most one tile with these categories and heights."""
    n = len(z)
    assert 1 <= n <= TILE, "only the path of a one-tile list is a function of its keys"
    if n <= WAVE_MAX:
        return "wave"
    if n > BUCKET_TILE:
        return "network:above 4032"
    if cloud_order:  # the key is the cloud index alone: every height field is zero
        return "network:one height"
    if len(np.unique(cat)) > 1:
        return "network:categories"
    z = canonical(z)
    if not np.isfinite(z).all():
        return "network:non-finite"
    if z.min() == z.max():
        return "network:one height"
    most, _ = fullest_bucket(z)
    if most is None:
        return "network:scale"
    return "network:skew" if most > MAX_BUCKET else "bucket"


def network_size(n):
    """keys the bitonic network sorts for a tile of n: the next power of two"""
    return 1 << max(n - 1, 0).bit_length()


def tiles_and_passes(n):
    tiles = (n + TILE - 1) // TILE
    return tiles, (tiles - 1).bit_length()


# ---------------------------------------------------------------------------------------------------------------
# the clouds
# ---------------------------------------------------------------------------------------------------------------
def bin_limits(p, zone, ring, sector):
    """(r0, r1, theta0, theta1) of a CZM bin, as the reference's constructor computes them (patchworkpp.h:122-134)."""
    mn, mx = p.min_range, p.max_range
    starts = [mn, (7 * mn + mx) / 8.0, (3 * mn + mx) / 4.0, (mn + mx) / 2.0, mx]
    size = (starts[zone + 1] - starts[zone]) / p.num_rings_each_zone[zone]
    width = 2 * math.pi / p.num_sectors_each_zone[zone]
    return starts[zone] + ring * size, starts[zone] + (ring + 1) * size, sector * width, (sector + 1) * width


COLUMN_BIN = (1, 0, 1)   # zone 1: R-VPF never strips there; concentric ring 2
FLOOR_BIN = (1, 2, 1)    # concentric ring 4: an upright patch beyond the rings of interest is ground without further tests
WALL_BIN = (0, 1, 0)     # zone 0: R-VPF strips what lies on a vertical seed plane


def _polar(rng, lim, n, margin=0.25):
    r0, r1, t0, t1 = lim
    r = rng.uniform(r0 + margin, r1 - margin, n)
    t = rng.uniform(t0 + 0.02, t1 - 0.02, n)
    return r * np.cos(t), r * np.sin(t)


def _rows(x, y, z):
    pts = np.empty((len(z), 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3] = x, y, z, 0.5  # (intensity 0.5: too bright for RNR)
    return pts


def _floor(rng, p, which, n, base=-SENSOR_HEIGHT):
    x, y = _polar(rng, bin_limits(p, *which), n)
    return _rows(x, y, base + rng.uniform(-0.03, 0.03, n))


def _column(rng, p, which, heights):
    r0, r1, t0, t1 = bin_limits(p, *which)
    r = 0.5 * (r0 + r1) + rng.uniform(-0.02, 0.02, len(heights))
    t = 0.5 * (t0 + t1) + rng.uniform(-0.002, 0.002, len(heights))
    return _rows(r * np.cos(t), r * np.sin(t), heights)


def _shuffled(rng, blocks, chosen_block):
    """Rows of all blocks in one shuffled cloud; the new indices of the rows of blocks[chosen_block], ascending."""
    pts = np.concatenate(blocks, axis=0)
    mark = np.concatenate([np.full(len(b), k == chosen_block) for k, b in enumerate(blocks)])
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), np.nonzero(mark[perm])[0]


def spread(n, lo=-1.0, hi=3.0):
    """n distinct float32 heights spread evenly"""
    h = np.linspace(lo, hi, n).astype(np.float32) if n > 1 else np.array([0.5 * (lo + hi)], np.float32)
    assert len(np.unique(h)) == n
    return h


def with_signed_zeros(pts, chosen, count):
    """`count` of the chosen rows get z = +0.0, -0.0, +0.0 ... alternating in cloud index."""
    rows = chosen[:: max(1, len(chosen) // count)][:count]
    assert len(rows) == count
    pts[rows, 2] = np.where(np.arange(count) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    assert np.signbit(pts[rows, 2]).sum() == count // 2
    return pts


def column_cloud(p, heights, seed):
    """A non-ground part of category 255 with exactly these heights (all above -1.4 m): a column over a floor of 64 points."""
    rng = np.random.default_rng([seed, len(heights)])
    heights = np.asarray(heights, np.float32)
    assert (heights > -1.4).all()
    return _shuffled(rng, [_floor(rng, p, COLUMN_BIN, FLOOR_POINTS), _column(rng, p, COLUMN_BIN, heights)], 1)


def floor_cloud(p, offsets, seed, base=-SENSOR_HEIGHT):
    """A ground part of exactly len(offsets) entries (at least 10): a floor at base + offsets, |offsets| <= 0.03 m."""
    rng = np.random.default_rng([seed, len(offsets)])
    offsets = np.asarray(offsets, np.float64)
    assert len(offsets) >= 10 and np.abs(offsets).max() <= 0.03
    x, y = _polar(rng, bin_limits(p, *FLOOR_BIN), len(offsets))
    return _shuffled(rng, [_rows(x, y, (base + offsets).astype(np.float32))], 0)


def pseudo_cloud(p, n, seed, near=False):
    """A pseudo-bin of exactly n entries: points beyond max_range (or inside min_range), next to a floor and a short column."""
    rng = np.random.default_rng([seed, n])
    r = rng.uniform(0.3, p.min_range - 0.2, n) if near else rng.uniform(p.max_range + 5.0, p.max_range + 30.0, n)
    t = rng.uniform(0.0, 2 * math.pi, n)
    out = _rows(r * np.cos(t), r * np.sin(t), rng.uniform(-2.0, 3.0, n).astype(np.float32).round(1))  # (heights repeat: they must not matter)
    return _shuffled(rng, [_floor(rng, p, COLUMN_BIN, FLOOR_POINTS), _column(rng, p, COLUMN_BIN, spread(20)), out], 2)


def small_bin_cloud(p, seed):
    """A bin of nine points (fewer than num_min_pts): a part in cloud order."""
    rng = np.random.default_rng([seed, 9])
    x, y = _polar(rng, bin_limits(p, 2, 1, 3), 9)
    return _shuffled(rng, [_floor(rng, p, COLUMN_BIN, FLOOR_POINTS), _rows(x, y, rng.uniform(-1.8, 2.0, 9))], 1)


def wall_cloud(p, n_wall, n_column, seed):
    """A non-ground part of two categories in a zone-0 bin: a thin wall that reaches below the floor owns the lowest points, so the
    seed plane of R-VPF round 1 is vertical and the round removes the wall (category 1); the floor then gives an upright plane, and
    a column elsewhere in the bin is what the final split leaves (category 255).  Chosen: wall and column."""
    rng = np.random.default_rng([seed, n_wall, n_column])
    r0, r1, t0, t1 = bin_limits(p, *WALL_BIN)
    rc, tc = 0.5 * (r0 + r1), 0.5 * (t0 + t1)
    # the wall: in the plane through (rc, tc) perpendicular to the ray, 1 m wide, from -2.05 m (above the seed margin -1.2 h) to -0.5 m
    s = rng.uniform(-0.5, 0.5, n_wall)
    wx = rc * math.cos(tc) - s * math.sin(tc) + rng.uniform(-0.003, 0.003, n_wall)
    wy = rc * math.sin(tc) + s * math.cos(tc)
    wall = _rows(wx, wy, spread(n_wall, -2.05, -0.5))
    fx, fy = _polar(rng, (r0, rc - 0.8, t0, t1), FLOOR_POINTS)
    floor = _rows(fx, fy, -SENSOR_HEIGHT + rng.uniform(-0.03, 0.03, FLOOR_POINTS))
    cr = rc + 1.2 + rng.uniform(-0.02, 0.02, n_column)
    ct = tc + rng.uniform(-0.002, 0.002, n_column)
    column = _rows(cr * np.cos(ct), cr * np.sin(ct), spread(n_column, -1.0, 3.0))
    pts = np.concatenate([floor, wall, column], axis=0)
    mark = np.arange(len(pts)) >= FLOOR_POINTS
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), np.nonzero(mark[perm])[0]


def whole_bin_cloud(p, heights, seed):
    """With seed and distance thresholds beyond the floats (ALL_GROUND_VARIANT) every point of a patch enters every fit and passes
    the plane test: floor and `heights` are ONE part of category 0, whatever the heights and whichever list the patch's decision
    sends its ground candidates to.  Chosen: all of it."""
    rng = np.random.default_rng([seed, len(heights)])
    pts = np.concatenate([_floor(rng, p, FLOOR_BIN, FLOOR_POINTS), _column(rng, p, FLOOR_BIN, np.asarray(heights, np.float32))], axis=0)
    perm = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[perm]), np.arange(len(pts))


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """name; the list and the exact length of the part under test; parameter variant (fields of the parameter block); builder"""

    def __init__(self, name, which, length, make, variant=None):
        self.name, self.which, self.length, self._make, self.variant = name, which, length, make, dict(variant or {})
        self._built = None

    def cloud(self, p):
        """(pts, chosen): the frame and the cloud indices of the points the part under test consists of"""
        if self._built is None:
            self._built = self._make(p)
        return self._built

    def __repr__(self):
        return self.name


GROUND_LENGTHS = (64, 128, 256, 257, 513, 4031, 4032, 4033, 4096, 4097, 8193, 16385)
COLUMN_LENGTHS = (1, 2, 63, 65, 129, 255, 256, 257, 512, 4032, 4033, 4095, 4096, 4097, 8192, 12289, 32769)
FAR_LENGTHS = (256, 257, 4096, 4097, 8193, 20000)
ZERO_VARIANT = dict(sensor_height=0.0)   # the sensor at floor level: the floor lies at z = +-0.0
ALL_GROUND_VARIANT = dict(th_seeds=1e39, th_seeds_v=1e39, th_dist=1e39)  # beyond the floats: every point of a patch is a seed and passes the plane test


def _tied(levels, per_level, extra=0):
    """`levels` distinct heights 0.25 m apart, `per_level` entries each, the first with `extra` more"""
    h = np.repeat(np.arange(levels, dtype=np.float32) * np.float32(0.25), per_level)
    return np.concatenate([h, np.zeros(extra, np.float32)])


def _one_ulp_pair(n):
    h = spread(n)
    h[n // 2 + 1] = np.nextafter(h[n // 2], np.float32(np.inf))  # (two keys that differ in the last bit of the height)
    assert len(np.unique(h)) == n
    return h


def _with(h, *values):
    h = np.array(h, np.float32)
    h[: len(values)] = values
    return h


def _zeros_in_column(n, count, seed):
    def make(p):
        pts, chosen = column_cloud(p, spread(n), seed)
        return with_signed_zeros(pts, chosen, count), chosen
    return make


def _zeros_in_floor(n, count, seed):
    def make(p):
        pts, chosen = floor_cloud(p, np.linspace(-0.03, 0.03, n), seed, base=0.0)
        return with_signed_zeros(pts, chosen, count), chosen
    return make


def make_cases():
    c = []
    for n in GROUND_LENGTHS:
        c.append(Case("spread-ground-%d" % n, "ground", n, lambda p, n=n: floor_cloud(p, np.linspace(-0.03, 0.03, n), 100)))
    for n in COLUMN_LENGTHS:
        c.append(Case("spread-column-%d" % n, "nonground", n, lambda p, n=n: column_cloud(p, spread(n), 200)))
    # declined by the distribution sort (and, for contrast, accepted with ties in every bucket)
    c.append(Case("one-height-300", "nonground", 300, lambda p: column_cloud(p, np.full(300, 0.75, np.float32), 300)))
    c.append(Case("one-height-2100", "nonground", 2100, lambda p: column_cloud(p, np.full(2100, 0.75, np.float32), 301)))
    c.append(Case("ties-16x32", "nonground", 512, lambda p: column_cloud(p, _tied(16, 32), 302)))
    c.append(Case("ties-16x32-and-one-of-33", "nonground", 513, lambda p: column_cloud(p, _tied(16, 32, 1), 303)))
    c.append(Case("two-categories-1100", "nonground", 1100, lambda p: wall_cloud(p, 700, 400, 304)))
    c.append(Case("one-ulp-apart-600", "nonground", 600, lambda p: column_cloud(p, _one_ulp_pair(600), 305)))
    # (the fit clamps heights to z0 +- 32 m: the two points at -3e38 tilt the plane, the patch is not upright and its ground
    # candidates -- one part of category 0 -- go to the non-ground list)
    c.append(Case("range-overflows-2100", "nonground", 2100 + FLOOR_POINTS,
                  lambda p: whole_bin_cloud(p, _with(spread(2100), 3e38, -3e38, 3e38, -3e38), 306), ALL_GROUND_VARIANT))
    c.append(Case("plus-infinity-4000", "nonground", 4000, lambda p: column_cloud(p, _with(spread(4000), np.inf, np.inf), 307)))
    # signed zeros
    c.append(Case("zeros-column-200", "nonground", 200, _zeros_in_column(200, 60, 400)))
    c.append(Case("zeros-column-700", "nonground", 700, _zeros_in_column(700, 24, 401)))
    c.append(Case("zeros-column-1000", "nonground", 1000, _zeros_in_column(1000, 300, 402)))
    c.append(Case("zeros-column-5000", "nonground", 5000, _zeros_in_column(5000, 400, 403)))
    c.append(Case("zeros-ground-500", "ground", 500, _zeros_in_floor(500, 100, 404), ZERO_VARIANT))
    # parts in cloud order
    for n in FAR_LENGTHS:
        c.append(Case("beyond-max-range-%d" % n, "nonground", n, lambda p, n=n: pseudo_cloud(p, n, 500)))
    c.append(Case("inside-min-range-4097", "nonground", 4097, lambda p: pseudo_cloud(p, 4097, 501, near=True)))
    c.append(Case("small-bin-9", "nonground", 9, lambda p: small_bin_cloud(p, 502)))
    return c


CASES = make_cases()


def configured(p, variant):
    """the parameter block with a case's variant applied (plain fields only)"""
    for k, v in variant.items():
        setattr(p, k, v)
    return p


def part_under_test(result, chosen):
    """(which, ordinal, positions) of the part of the oracle's lists that holds the chosen points -- all of them, nothing else."""
    chosen = np.asarray(chosen)
    for which, idx, part in (("ground", result.ground_idx, result.ground_part), ("nonground", result.nonground_idx, result.nonground_part)):
        pos = np.nonzero(idx == chosen[0])[0]
        if len(pos):
            at = np.nonzero(part == part[pos[0]])[0]
            assert np.array_equal(np.sort(idx[at]), np.sort(chosen)), "the part under test is not the chosen points: %d entries, %d chosen" % (len(at), len(chosen))
            return which, int(part[pos[0]]), at
    raise AssertionError("the chosen points are in neither list")


def describe(case, pts, chosen, result):
    """One row of the case table: what the part under test is and which path K7 takes for it."""
    which, ordinal, at = part_under_test(result, chosen)
    idx, cat, cloud = ((result.ground_idx, result.ground_cat, result.ground_part_cloud) if which == "ground"
                       else (result.nonground_idx, result.nonground_cat, result.nonground_part_cloud))
    z, cats, in_cloud_order = pts[idx[at], 2], cat[at], bool(cloud[ordinal])
    n = len(at)
    tiles, passes = tiles_and_passes(n)
    heights = 1 if in_cloud_order else len(np.unique(canonical(z)))
    most = None
    if not in_cloud_order and np.isfinite(z).all() and heights > 1:
        most = fullest_bucket(z)[0]
    path = sort_path(cats, z, in_cloud_order) if n <= TILE else "tiles"
    return dict(case=case.name, list=which, length=n, categories=sorted(set(int(c) for c in cats)), cloud_order=in_cloud_order, heights=heights,
                fullest=most, path=path, network=network_size(n) if path.startswith("network") else 0, tiles=tiles, passes=passes)
