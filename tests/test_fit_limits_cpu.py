"""The saturated patches of fit_limits_ref.py on the CPU: the construction saturates what it claims to (preconditions on the
input), the restatement puts every point into the final plane, and its plane equals the big-integer anchor bit for bit --
the one check in the suite that does not compare two texts of one author against each other: the anchor's moments are
Python's integers."""
from fractions import Fraction

import numpy as np
import pytest

import fit_limits_ref as fl
import oracle_lib as ol

E_S8 = fl.effective_edge("S8:65535")
SIZES = (2047, 2048, E_S8, E_S8 + 1, 65535, 65536, 458751, 458752)
COMBOS = [(g, az, zl, wide) for g in "AB" for az in fl.AZIMUTHS_OF[g] for zl in fl.ZLOWS for wide in (True, False)]


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


def run_case(oracle, geometry, azimuth, zlow, wide, n):
    est = ol.Estimator(oracle, fl.configure(oracle.default_params(), geometry), arith=ol.ARITH_FXP if wide else ol.ARITH_FXP21)
    shift, zr, ox, oy = est.fxp_geometry()
    g = fl.GEOMETRIES[geometry]
    assert (shift, zr) == (g["shift"][wide], g["zr"])
    if geometry == "A":  # fewer than four sectors: the sensor is every bin's origin
        assert not ox.any() and not oy.any()
    else:
        assert (ox[g["bin"]], oy[g["bin"]]) == (48.375, 48.375)
    pts = fl.cloud(geometry, azimuth, zlow, n)
    res = est.run(pts)
    rec = fl.patch_of(res.records, geometry)
    anchor = fl.Anchor(pts, shift, wide, (ox[g["bin"]], oy[g["bin"]]), fl.z_origin(pts))
    fl.check_preconditions(geometry, azimuth, zlow, anchor)
    assert int(rec["n_ground"]) == n
    anchor.assert_equals_record(rec, n)
    return pts, anchor


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("geometry,azimuth,zlow,wide", COMBOS, ids=["%s-%s-%s-%s" % (g, az, zl, "wide" if w else "narrow") for g, az, zl, w in COMBOS])
def test_saturated_patch_restatement_equals_anchor(oracle, geometry, azimuth, zlow, wide, n):
    run_case(oracle, geometry, azimuth, zlow, wide, n)


def test_largest_frame_on_the_wide_grid(oracle):
    """4 194 304 points in one bin, x and z saturated: S2 near 2^92, covariance numerators of about 100 bits."""
    _, anchor = run_case(oracle, "A", "x-", "reach", True, fl.MAX_POINTS)
    assert max(abs(anchor.s2[0][0]), abs(anchor.s2[0][2])).bit_length() >= 91 and anchor.numerator_bits >= 96


def test_quantiser_and_limb_sums_against_rationals_and_python_integers(oracle):
    """The two vectorised steps of the anchor against their plainest form: Q against Fractions (values that round on the grid:
    |v| < 2^-5 m on the narrow one, ties included), the three-limb sums against sums of Python ints."""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.normal(0, 1e-3, 300), rng.normal(0, 40, 300), (np.arange(-64, 64) + 0.5) * 2.0 ** -19,
                        [0.0, -0.0, 1e-30, -1e-30, 127.9, -127.9]]).astype(np.float32)
    for origin, shift in ((0.0, 28), (0.0, 19), (48.375, 29), (-129.125, 19), (-141.75, 28), (2.5, 3)):
        q = fl.quantise(v, origin, shift)
        assert q.tolist() == [fl.quantise_fraction(x, origin, shift) for x in v]
    pts = fl.cloud("A", "diag", "clamp", (1 << 17) + 5)
    a = fl.Anchor(pts, 28, True, (0.0, 0.0), fl.z_origin(pts))
    cols = [a.q[:, k].tolist() for k in range(3)]
    assert a.s1 == [sum(c) for c in cols]
    for i in range(3):
        for j in range(3):
            assert a.s2[i][j] == sum(x * y for x, y in zip(cols[i], cols[j]))
    assert Fraction(a.s2[0][1], len(pts)) > 2 ** 67  # (x and y of one sign at 0.71 of the range each)


def test_effective_edges_against_a_scan_of_the_bucket_functions():
    """A plan entry takes the buckets below the bucket of (upper + 1): its largest patch is one less than that bucket's
    smallest size.  size_bucket / bucket_floor are scanned by brute force: monotone, floor(bucket(n)) <= n, and the floor is
    the first n of its bucket."""
    first = {}
    last = 0
    for n in range(1, 1 << 20):
        b = fl.size_bucket(n)
        assert b >= last
        last = b
        first.setdefault(b, n)
    for b, n in first.items():
        assert fl.bucket_floor(b) == n
    expect = {"W16:65535": 2047, "W16.16:65535": 2047, "W16.32:65535": 2047, "S8:65535": 14335, "S16:65535": 28671, "S32:65535": 57343,
              "S64:65535": 65535, "W64.2:65535": 65535, "W64.4:65535": 65535, "W64.8:65535": 65535, "W64.16:65535": 65535,
              "B64:600000": 458751, "H64:511": 458751}
    for entry, e in expect.items():
        mode, lanes, _, upper = fl.plan_entry(entry)
        cap = fl.lane_cap(mode, lanes)
        upper = cap if mode == "H" else min(upper, cap, 65535 if mode not in "BH" else cap)
        assert fl.effective_edge(entry) == e == first[fl.size_bucket(upper + 1)] - 1, entry
        # the lane bound the caps are there for: no lane of a patch of that size, stored in one part or split in two, adds more than 2047
        # (and the bound pwpp_launch_fit states for it: n / G + 16, n / 256 + 24 with four waves)
        bound = e // 256 + 24 if mode in "BH" else e // lanes + 16
        for parts in ((e, 0), (e // 2, e - e // 2), (1, e - 1), (e - 1, 1)):
            assert fl.max_lane_points(mode, lanes, parts) <= bound <= 2047, (entry, parts)
