"""Saturated patches for the plane-fit sums, and an anchor in Python integers (TEST INFRASTRUCTURE, numpy only).

The fit kernels' bounds (pwpp_fit.hip, pwpp_common.hpp: 2047 products of 2^52 per lane, the class caps of pwpp_launch_fit,
the 64 / 128-bit switch of the row sums, the joins of two halves) are tight only where the quantised coordinates use the
whole width of the contract: |Q| near 2^35, or 2^26 on the narrow grid.  No scan comes near that, so the clouds are built:

GEOMETRY A  one sector and one ring per zone (fewer than four sectors: the sensor stays the origin of every bin),
            min_range 2.7, max_range 127.98: shift 28 on the wide grid, 19 on the narrow one, ZR = 128 m.
GEOMETRY B  four sectors and one ring per zone, max_range 90.25: shift 29 / 20, ZR = 64 m, bin-centred origins; the slab
            sits at the far corner (r = max_range, azimuth 0+) of sector 0 of zone 3, 48.375 m from its origin in y.

A frame holds n points in ONE bin of zone 3: point 0, the only low point, at `zlow`, and a thin slab (1.9 m in range, +-0.01
rad, z = -1.7 + N(0, 0.01)) around the same azimuth.  num_lpr = 1 makes the low point the patch's z origin, th_seeds =
th_dist = 1000 put every point into every fit set: the final plane is the plane of all n points and n_ground = n.
  zlow = -1.7 - 0.9953125 ZR   every slab point at 0.996 of the range in z, unclamped   ("reach";  A: -1.7 - 127.4)
  zlow = -1.7 - ZR - 12        every slab point clamped to exactly Q_z = 2^35 (2^26)     ("clamp";  A: -1.7 - 140)

THE ANCHOR  from the cloud and the shift, origins and z0 the library reports: Q in exact integers, S1 and S2 as Python
ints, mean and covariance as pwpp_common.hpp states them (one float(int), correctly rounded, per numerator), the oracle's
Jacobi on that float covariance, normal and d.  It shares no summation code with the kernels or with the restatement.
"""
import math
from fractions import Fraction

import numpy as np

import oracle_lib as ol

NUM_BUCKETS = 96  # PWPP_NUM_BUCKETS
MAX_POINTS = 4194304  # the largest frame the C-ABI accepts

GEOMETRIES = {
    "A": dict(sectors=1, max_range=127.98, shift={True: 28, False: 19}, zr=128.0, bin=3),
    "B": dict(sectors=4, max_range=90.25, shift={True: 29, False: 20}, zr=64.0, bin=12),
}
# geometry A: both signs of Q_x and Q_y alone, and both at once (|Q_x Q_y| ~ 2^69); geometry B: the corner of the bin
AZIMUTHS = {"x+": 0.0, "y+": 0.5 * math.pi, "x-": math.pi, "y-": 1.5 * math.pi, "diag": 1.25 * math.pi}
AZIMUTHS_OF = {"A": ("x+", "y+", "x-", "y-", "diag"), "B": ("corner",)}
ZLOWS = ("reach", "clamp")


def configure(p, geometry):
    """Set the fields of a parameter block (pwpp_hip.Params or oracle_lib.Params) for geometry "A" or "B"."""
    g = GEOMETRIES[geometry]
    for k in range(4):
        p.num_sectors_each_zone[k] = g["sectors"]
        p.num_rings_each_zone[k] = 1
    p.min_range = 2.7
    p.max_range = g["max_range"]
    p.num_lpr = 1
    p.th_seeds = 1000.0
    p.th_dist = 1000.0
    p.enable_RNR = 0
    p.num_min_pts = 10
    return p


def zlow_of(geometry, zlow):
    zr = GEOMETRIES[geometry]["zr"]
    return -1.7 - 0.9953125 * zr if zlow == "reach" else -1.7 - zr - 12.0


def cloud(geometry, azimuth, zlow, n):
    """(n, 4) float32: point 0 the low point, n - 1 slab points; deterministic in its arguments."""
    g = GEOMETRIES[geometry]
    rng = np.random.default_rng([ord(geometry), sorted(AZIMUTHS).index(azimuth) if azimuth in AZIMUTHS else 9, n])
    if geometry == "A":
        az0, r_low, r0, r1, half = AZIMUTHS[azimuth], 127.0, 126.0, 127.9, 0.01
    else:  # (azimuth 0 itself belongs to the LAST sector: the slab stays above it)
        az0, r_low, r0, r1, half = 0.011, 89.25, 88.35, 90.15, 0.01
    r = np.concatenate([[r_low], rng.uniform(r0, r1, n - 1)])
    az = np.concatenate([[az0], az0 + rng.uniform(-half, half, n - 1)])
    z = np.concatenate([[zlow_of(geometry, zlow)], -1.7 + rng.normal(0.0, 0.01, n - 1)])
    pts = np.zeros((n, 4), np.float32)
    pts[:, 0] = r * np.cos(az)
    pts[:, 1] = r * np.sin(az)
    pts[:, 2] = z
    assert float(np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)).max()) < g["max_range"]
    assert pts[0, 2] < pts[1:, 2].min() - 1.0  # the one low point
    return pts


# ---------------------------------------------------------------------------------------------------------------
# the size classes (pwpp_common.hpp: pwpp_size_bucket, pwpp_bucket_floor; pwpp_fit.hip: pwpp_launch_fit)
# ---------------------------------------------------------------------------------------------------------------
def size_bucket(n):
    if n < 4:
        return n
    e = n.bit_length() - 1
    return min(4 * e + ((n >> (e - 2)) & 3) - 4, NUM_BUCKETS - 1)


def bucket_floor(b):
    if b < 4:
        return max(b, 1)
    e, q = divmod(b + 4, 4)
    return (1 << e) + (q << (e - 2))


def plan_entry(entry):
    """"S8:65535" -> ('S', 8, 0, 65535), "W64.4:65535" -> ('W', 64, 4, 65535)"""
    head, upper = entry.split(":")
    lanes, _, per_wave = head[1:].partition(".")
    return head[0], int(lanes), int(per_wave or 0), int(upper)


def lane_cap(mode, lanes):
    return 2023 * 256 if mode in "BH" else (2047 if mode == "W" and lanes == 16 else 2031 * lanes)


def effective_edge(entry):
    """The largest patch a plan entry really takes: its range ends where the bucket of (upper + 1) begins."""
    mode, lanes, _, upper = plan_entry(entry)
    upper = min(upper, lane_cap(mode, lanes))
    if mode not in "BH":
        upper = min(upper, 65535)
    if mode == "H":  # four waves per patch above `upper`, up to the cap of the four-waves kernel
        upper = lane_cap(mode, lanes)
    return bucket_floor(size_bucket(upper + 1)) - 1


def max_lane_points(mode, lanes, parts):
    """The most points one lane adds up when a patch stored in `parts` (points of the low part, of the high part) is dealt as
    pwpp_fit.hip states it: chunks of 8 points per lane of a row of `lanes` lanes, numbered through the low part and then the
    high part; lanes < 64: slot k of lane j = point 8 G c + k G + j; 64 lanes: four consecutive points twice per chunk (4 j + k
    % 4, + 256 for k >= 4); mode 'B' / 'H': wave w of four takes the chunks c = w, w + 4, ...  Lane 0 holds the most of every
    chunk, so lane 0 of the busiest wave is the answer."""
    per_chunk = []
    for n in parts:
        for c in range((n + 8 * lanes - 1) // (8 * lanes)):
            rem = n - 8 * lanes * c
            if lanes == 64:
                per_chunk.append(min(4, rem) + min(4, max(0, rem - 256)))
            else:
                per_chunk.append(min(8, (rem + lanes - 1) // lanes))
    waves = 4 if mode in "BH" else 1
    return max(sum(per_chunk[w::waves]) for w in range(waves))


# ---------------------------------------------------------------------------------------------------------------
# the anchor
# ---------------------------------------------------------------------------------------------------------------
def quantise_fraction(v, origin, shift):
    """Q of ONE value, in rationals: round-half-even(v 2^s - origin 2^s) (Python rounds a Fraction to the even neighbour)."""
    return round(Fraction(float(v)) * 2 ** shift - Fraction(float(origin)) * 2 ** shift)


def quantise(v, origin, shift):
    """Q of a float32 array as int64, in integers: v = m 2^e with a 24-bit m; origin 2^s is an integer (a multiple of 1/8 m,
    s >= 3), so it does not take part in the rounding."""
    o = Fraction(float(origin)) * 2 ** shift
    assert o.denominator == 1 and abs(o) < 2 ** 40
    assert v.dtype == np.float32 and np.isfinite(v).all()
    m, e = np.frexp(v.astype(np.float64))
    m = np.ldexp(m, 24).astype(np.int64)  # exact: |m| < 2^24
    sh = e.astype(np.int64) - 24 + shift
    assert sh.max() <= 38
    up = m << np.maximum(sh, 0)
    k = np.minimum(np.maximum(-sh, 1), 26)  # (2^-26 |m| < 1/4: the nearest integer is 0 from there on)
    fl = m >> k
    rem = m - (fl << k)
    half = np.int64(1) << (k - 1)
    down = fl + ((rem > half) | ((rem == half) & ((fl & 1) == 1)))
    return np.where(sh >= 0, up, down) - int(o)


def exact_sums(q):
    """(S1[3], S2[3][3]) of an (n, 3) int64 array as Python ints.  Up to 2^17 points: Python's own integers, nothing else.
    Above: three limbs of numpy int64 sums that cannot overflow (q = a 2^20 + b, |a| <= 2^15, 0 <= b < 2^20, n <= 2^22:
    |sum a a| <= 2^52, |sum a b| <= 2^57, sum b b < 2^62), put together in Python ints."""
    n = q.shape[0]
    assert np.abs(q).max() <= 2 ** 35 and n <= 1 << 22
    s1 = [int(q[:, a].sum()) for a in range(3)]  # |S1| <= 2^57
    s2 = [[0] * 3 for _ in range(3)]
    if n <= 1 << 17:
        cols = [q[:, a].tolist() for a in range(3)]
        assert s1 == [sum(c) for c in cols]
        for a in range(3):
            for b in range(a, 3):
                s2[a][b] = s2[b][a] = sum(x * y for x, y in zip(cols[a], cols[b]))
        return s1, s2
    hi, lo = q >> 20, q & ((1 << 20) - 1)
    for a in range(3):
        for b in range(a, 3):
            hh = int((hi[:, a] * hi[:, b]).sum())
            hl = int((hi[:, a] * lo[:, b]).sum()) + int((lo[:, a] * hi[:, b]).sum())
            ll = int((lo[:, a] * lo[:, b]).sum())
            s2[a][b] = s2[b][a] = (hh << 40) + (hl << 20) + ll
    return s1, s2


class Anchor:
    """The plane of ALL points of `pts` under the contract, from (shift, wide, the bin's origin, z0)."""

    def __init__(self, pts, shift, wide, origin_xy, z0):
        n = pts.shape[0]
        qmax = 2 ** 35 if wide else 2 ** 26
        zr = Fraction(qmax, 2 ** shift)
        org = [float(origin_xy[0]), float(origin_xy[1]), float(z0)]
        zlo, zhi = np.float32(float(z0 - zr)), np.float32(float(z0 + zr))
        assert Fraction(float(zlo)) == Fraction(z0) - zr and Fraction(float(zhi)) == Fraction(z0) + zr  # exact in float
        zc = np.minimum(np.maximum(pts[:, 2], zlo), zhi)
        self.clamped = bool((zc != pts[:, 2]).any())
        q = np.stack([quantise(pts[:, 0].copy(), org[0], shift), quantise(pts[:, 1].copy(), org[1], shift), quantise(zc, org[2], shift)], axis=1)
        self.q = q
        self.qmax = qmax
        self.reach = tuple(float(np.abs(q[:, a]).max()) / qmax for a in range(3))
        self.q_min = tuple(int(q[:, a].min()) for a in range(3))
        self.q_max = tuple(int(q[:, a].max()) for a in range(3))
        s1, s2 = exact_sums(q)
        self.s1, self.s2 = s1, s2
        inv = 2.0 ** -shift
        rn, rd = 1.0 / float(n), 1.0 / (float(n) * float(n - 1))
        self.mean = np.array([np.float32((float(s1[a]) * rn) * inv + org[a]) for a in range(3)], np.float32)
        self.numerator_bits = max((n * s2[a][b] - s1[a] * s1[b]).bit_length() for a in range(3) for b in range(3))
        self.cov = np.array([[np.float32((float(n * s2[a][b] - s1[a] * s1[b]) * rd) * (inv * inv)) for b in range(3)] for a in range(3)],
                            np.float32)
        u, sv = ol.jacobi(self.cov)
        normal = u[:, 2].copy()
        if normal[2] < 0:
            normal = normal * np.float32(-1)
        self.normal, self.sv = normal, sv
        dot = normal[0] * self.mean[0] + normal[1] * self.mean[1] + normal[2] * self.mean[2]  # float products, float adds, left to right
        assert dot.dtype == np.float32
        self.d = float(-dot)

    def assert_equals_record(self, rec, n):
        """Bitwise: mean, singular values, normal and d of a patch record (oracle_lib / pwpp_hip RECORD_DTYPE)."""
        assert int(rec["n_points"]) == n and int(rec["n_ground"]) == n, (int(rec["n_points"]), int(rec["n_ground"]), n)
        for name, mine in (("mean", self.mean), ("sv", self.sv), ("normal", self.normal)):
            got = np.asarray(rec[name], np.float32)
            assert got.tobytes() == mine.tobytes(), "%s: record %r, anchor %r" % (name, got, mine)
        assert np.float64(rec["d"]).tobytes() == np.float64(self.d).tobytes(), "d: record %r, anchor %r" % (rec["d"], self.d)


def check_preconditions(geometry, azimuth, zlow, anchor):
    """Conditions on the INPUT (not measurements of the code under test): the case saturates what it is there to saturate."""
    rx, ry, rz = anchor.reach
    if geometry == "A":
        if azimuth in ("x+", "x-"):
            assert rx >= 0.99
            assert (anchor.q_max[0] > 0) == (azimuth == "x+") and (anchor.q_min[0] < 0) == (azimuth == "x-")
        elif azimuth in ("y+", "y-"):
            assert ry >= 0.99
            assert (anchor.q_max[1] > 0) == (azimuth == "y+") and (anchor.q_min[1] < 0) == (azimuth == "y-")
        else:  # both at once, both negative: |Q_x Q_y| >= 2^68.9 per point of the far edge
            assert rx >= 0.69 and ry >= 0.69 and anchor.q_max[0] < 0 and anchor.q_max[1] < 0
    else:
        assert max(rx, ry) > 0.5  # 2^34 / 2^35: beyond anything the default geometry produces
    assert rz >= 0.99
    if zlow == "clamp":
        assert anchor.clamped and rz == 1.0
        assert int((anchor.q[:, 2] == anchor.qmax).sum()) == anchor.q.shape[0] - 1  # every slab point at exactly +2^35 (2^26)
    else:
        assert not anchor.clamped


def patch_of(records, geometry):
    """The record of the one occupied bin (and that it is the bin the construction aims at)."""
    big = records[records["n_points"] > 0] if len(records) > 1 else records
    assert len(big) == 1 and int(big[0]["bin"]) == GEOMETRIES[geometry]["bin"], records
    return big[0]


def z_origin(pts):
    """z0 of the patch: the first lowest-point representative (num_lpr = 1: the lowest z) rounded to 1/8 m, as the library's
    own exported helper rounds it."""
    return Fraction(ol.restatement().lib.pwo_ext_z_origin(float(pts[:, 2].min())))
