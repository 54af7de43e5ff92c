"""Every fit kernel at the largest patch its plan entry takes, and one point beyond, on SATURATED coordinates (fit_limits_ref.py:
|Q| at 0.99-1.0 of 2^35, or 2^26 with exact_moments = 0), on a real MI355X.  Each frame is compared bit for bit with the
restatement (assert_frame_equal) AND its big patch with the anchor in Python integers -- a lane that receives one point too
many, a sign lost in the split of Q = -2^35, a carry dropped between two halves or a 64 / 128-bit switch off by one gives a
wrong plane here and nowhere else in the suite.

The tests cannot observe which kernel ran: the routing (which entry takes which size) is covered by the restated bucket
functions alone (fit_limits_ref.effective_edge, checked against a scan in test_fit_limits_cpu.py).  A frame of E + 1 points
goes to the plan's next class, which is k_fit_stream where the plan has one entry.
"""
import numpy as np
import pytest

import fit_limits_ref as fl
import oracle_lib as ol
import pwpp_hip
from test_gpu_parity import assert_frame_equal, to_oracle_params

pytestmark = pytest.mark.gpu

WIDTHS = [pytest.param(True, id="wide"), pytest.param(False, id="narrow")]
# (geometry, azimuth, zlow) of the frame of E points and of the frame of E + 1: rotated over the plans of a family, so that every
# (family, width) sees a negative saturated Q_x, a saturated Q_y, the exact-clamp Q_z and geometry B
ROTATION = [
    ("A", ("x-", "clamp"), ("y+", "reach")),
    ("A", ("y-", "reach"), ("x+", "clamp")),
    ("B", ("corner", "clamp"), ("corner", "reach")),
    ("A", ("diag", "clamp"), ("x-", "reach")),
]
W16_PLANS = ["W16:65535", "W16.16:65535", "W16.32:65535"]
S_PLANS = ["S8:65535", "S16:65535", "S32:65535", "S64:65535"]
W64_PLANS = ["W64.2:65535", "W64.4:65535", "W64.8:65535", "W64.16:65535"]
BIG_PLANS = ["B64:600000", "H64:511"]
BIG_ROTATION = {"B64:600000": ROTATION[0], "H64:511": ROTATION[2]}


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


_CASES = {}
_ANCHORS = {}


def case(oracle, geometry, azimuth, zlow, n, wide):
    """(cloud, the restatement's result) of one frame, computed once per module."""
    key = (geometry, azimuth, zlow, n, wide)
    if key not in _CASES:
        p = to_oracle_params(fl.configure(pwpp_hip.default_params(), geometry))
        est = ol.Estimator(oracle, p, arith=ol.ARITH_FXP if wide else ol.ARITH_FXP21)
        pts = fl.cloud(geometry, azimuth, zlow, n)
        ref = est.run(pts)
        assert int(fl.patch_of(ref.records, geometry)["n_ground"]) == n
        _CASES[key] = (pts, ref)
    return _CASES[key]


def make_handle(geometry, wide, plan):
    h = pwpp_hip.Handle(fl.configure(pwpp_hip.default_params(), geometry))
    if not wide:
        h.set_option("exact_moments", 0)
    h.set_option("fit_plan", plan)
    assert h.fxp_shift() == fl.GEOMETRIES[geometry]["shift"][wide]
    return h


def run_and_check(h, oracle, geometry, wide, frames, what=""):
    """One estimate_ground_batch call on `frames` = [(azimuth, zlow, n), ...]: every frame against the restatement, its big patch
    against the anchor built from what the HANDLE reports (shift, origins), the clamp counter."""
    before = h.clamped_frames()
    got = [case(oracle, geometry, az, zl, n, wide) for az, zl, n in frames]
    h.estimate_ground_batch([pts for pts, _ in got], mode=pwpp_hip.MODE_FRESH)
    origin = h.fxp_origins()[fl.GEOMETRIES[geometry]["bin"]]
    for k, ((az, zl, n), (pts, ref)) in enumerate(zip(frames, got)):
        try:
            assert_frame_equal(h, k, ref, n)
            akey = (geometry, az, zl, n, wide, h.fxp_shift(), float(origin[0]), float(origin[1]))
            if akey not in _ANCHORS:
                _ANCHORS[akey] = fl.Anchor(pts, h.fxp_shift(), wide, origin, fl.z_origin(pts))
            anchor = _ANCHORS[akey]
            fl.check_preconditions(geometry, az, zl, anchor)
            anchor.assert_equals_record(fl.patch_of(h.patch_records(k), geometry), n)
        except AssertionError as e:
            raise AssertionError("%s frame %d (%s %s %s, %d points, %s grid): %s" % (what, k, geometry, az, zl, n, "wide" if wide else "narrow", e)) from e
    assert h.clamped_frames() - before == sum(1 for _, zl, _ in frames if zl == "clamp")
    assert h.fixed_up_frames() == 0


def edge_pair(rotation, e):
    geometry, first, second = rotation
    return geometry, [first + (e,), second + (e + 1,)]


def split_in_halves(h, oracle, geometry, wide, frames):
    """Store every bin in two parts with the slab cut in the middle: the chunks are then dealt part by part, each part about
    half full (the split height is -sensor_height + hi_split: z = -1.7, the slab's median)."""
    hi_split = h.params.sensor_height - 1.7
    h.set_option("hi_split_zones", 4)
    h.set_option("hi_split", hi_split)
    zs = np.float32(-h.params.sensor_height + float(np.float32(hi_split)))
    for az, zl, n in frames:
        pts, _ = case(oracle, geometry, az, zl, n, wide)
        n_lo = int((pts[:, 2] < zs).sum())
        assert 0.4 * n < n_lo < 0.6 * n, (n_lo, n)


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("plan", W16_PLANS)
def test_sixteen_lane_rows_at_2047_points_per_patch(oracle, plan, wide):
    """k_fit_w64<16, .>: a row's totals stay in int64 up to 2047 points per PATCH (2047 products of 2^52); 2048 go on."""
    geometry, frames = edge_pair(ROTATION[W16_PLANS.index(plan)], fl.effective_edge(plan))
    assert frames[0][2] == 2047
    run_and_check(make_handle(geometry, wide, plan), oracle, geometry, wide, frames)


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("plan", S_PLANS)
def test_streaming_rows_at_their_largest_patch(oracle, plan, wide):
    """k_fit_srows<G>: the cap 2031 G ends at the bucket edge E (14 335 / 28 671 / 57 343 / 65 535); a second call with both stored
    parts half full."""
    geometry, frames = edge_pair(ROTATION[S_PLANS.index(plan)], fl.effective_edge(plan))
    h = make_handle(geometry, wide, plan)
    run_and_check(h, oracle, geometry, wide, frames)
    split_in_halves(h, oracle, geometry, wide, frames)
    run_and_check(h, oracle, geometry, wide, frames, "two parts:")


@pytest.mark.parametrize("plan", S_PLANS)
def test_streaming_rows_switch_to_128_bit_row_sums_above_2047_points(oracle, plan):
    """exact_moments = 0, |Q| = 2^26: a row of 2047 points sums its second moments in int64 (2047 * 2^52 fits), one of 2048 must
    not (`__any(n > 2047u)`).  All sizes lie inside the entry's class here.  One point of every patch is its z origin, so 2048
    points hold 2047 products of 2^52 at most: the third frame, 2049 points with 2048 of them clamped to exactly 2^26, is the
    smallest whose sum of Q_z^2 (2^63) does leave int64."""
    assert fl.effective_edge(plan) > 2049
    geometry, frames = edge_pair(ROTATION[(S_PLANS.index(plan) + 1) % 4], 2047)
    frames.append((frames[0][0], "clamp", 2049))
    h = make_handle(geometry, False, plan)
    run_and_check(h, oracle, geometry, False, frames)
    split_in_halves(h, oracle, geometry, False, frames)
    run_and_check(h, oracle, geometry, False, frames, "two parts:")


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("plan", W64_PLANS)
def test_big_bins_per_wave_at_65535_points(oracle, plan, wide):
    """k_fit_w64<64, 2 / 4 / 8 / 16>: one wave per patch up to 65 535 points (1024 per lane); a second call with both parts half full."""
    geometry, frames = edge_pair(ROTATION[W64_PLANS.index(plan)], fl.effective_edge(plan))
    assert frames[0][2] == 65535
    h = make_handle(geometry, wide, plan)
    run_and_check(h, oracle, geometry, wide, frames)
    split_in_halves(h, oracle, geometry, wide, frames)
    run_and_check(h, oracle, geometry, wide, frames, "two parts:")


def big_frames(plan):
    """E and E + 1 as everywhere; the family has two plans only, so geometry A brings its saturated Q_y in a third frame of E points
    (the frame of E + 1 is not the four-waves kernel's)."""
    geometry, frames = edge_pair(BIG_ROTATION[plan], fl.effective_edge(plan))
    if geometry == "A":
        frames.append(("y-", "reach", frames[0][2]))
    return geometry, frames


@pytest.mark.parametrize("wide", WIDTHS)
@pytest.mark.parametrize("plan", BIG_PLANS)
def test_four_waves_per_patch_at_458751_points(oracle, plan, wide):
    """k_fit_brows / k_fit_hybrid: the cap 2023 * 256 ends at the bucket edge 458 751 (1792 points per lane); 458 752 go to k_fit_stream."""
    geometry, frames = big_frames(plan)
    assert frames[0][2] == 458751
    run_and_check(make_handle(geometry, wide, plan), oracle, geometry, wide, frames)


def test_workgroup_kernel_alone_on_the_largest_frame(oracle):
    """k_fit_stream with its 128-bit lane sums: 4 194 304 points in one patch, x (negative) and z saturated, the wide grid.  The plan's
    one entry ("S8:0") takes no patch at all."""
    run_and_check(make_handle("A", True, "S8:0"), oracle, "A", True, [("x-", "reach", fl.MAX_POINTS)])


def mixed_frames(wide):
    """Every edge size of the plans above and the size beyond it, up to 458 752, the variants of geometry A dealt round."""
    sizes = sorted({e + k for plan in W16_PLANS + S_PLANS + W64_PLANS + BIG_PLANS for e in [fl.effective_edge(plan)] for k in (0, 1)})
    assert sizes == [2047, 2048, 14335, 14336, 28671, 28672, 57343, 57344, 65535, 65536, 458751, 458752]
    variants = [(az, zl) for az in fl.AZIMUTHS_OF["A"] for zl in fl.ZLOWS]
    return [variants[(3 * i + (0 if wide else 5)) % len(variants)] + (n,) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("wide", WIDTHS)
def test_launchers_own_plan_on_a_batch_of_all_edge_sizes(oracle, wide):
    """The empty plan (pwpp_launch_fit chooses by the batch's size) on one batch of every size above up to 458 752 (the 4 M frame
    stays alone: the capacities of a batch follow its largest frame)."""
    run_and_check(make_handle("A", wide, ""), oracle, "A", wide, mixed_frames(wide))
