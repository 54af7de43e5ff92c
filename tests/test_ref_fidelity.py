"""The restatement (oracle/pwpp_oracle.cpp) against the reference's own code (oracle/_ref: patchworkpp.cpp compiled unmodified,
in three arithmetic flavours) across the parameter space and the clouds of tools/fuzz_parity.py.

The GPU suite holds the HIP path bit for bit against the restatement on random parameter sets, stateful sequences and odd clouds
(test_randomised_differential_cases); test_oracle.py pins the restatement to the reference builds at default parameters only.
This file closes the gap between the two: for each seed, the fuzzer's parameter draw and a stateful sequence of 1-4 of its clouds
go through one object of the restatement and one of the reference build, flavour by flavour, and every output must be identical.
"""
import importlib.util
import math
import os

import numpy as np
import pytest

import oracle_lib as ol
import pwpp_synth

HERE = os.path.dirname(os.path.abspath(__file__))
ARITHS = [(ol.ARITH_EIGEN_F32, "eigen_f32"), (ol.ARITH_EXACT_F64, "exact_f64"), (ol.ARITH_F32_PACKET4, "f32_packet4")]
SEEDS = list(range(7000, 7040))


def _fuzzer():
    spec = importlib.util.spec_from_file_location("fuzz_parity_cpu", os.path.join(HERE, "..", "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def draw_case(fz, lib, seed):
    """(params, clouds) of one seed: the fuzzer's parameter draw on the restatement's Params, 1-4 of its clouds; every other seed
    adds the odd heights (+-inf, +-1e30, +-3e38, signed zeros, duplicates)."""
    rng = np.random.default_rng(seed)
    p = fz.random_params(rng, lib.default_params())
    odd = seed % 2 == 1
    # num_min_pts = 0 lets an EMPTY bin into the fit, and the reference's fit of an empty bin reads past its vectors: the reference
    # builds themselves segfault there (fuzz_parity seed 12) -- undefined behaviour of the reference, not a result to compare with.
    # The floor is 1 with the odd heights too: 100 odd-height seeds forced to num_min_pts 1, 2 and 3 matched all three builds.
    p.num_min_pts = max(p.num_min_pts, 1)
    saved = fz.ODD_HEIGHTS
    fz.ODD_HEIGHTS = odd  # (the module flag, not FUZZ_NO_ODD: the environment would change the GPU fuzz test's cases too)
    try:
        clouds = [fz.random_cloud(rng, p.sensor_height) for _ in range(int(rng.integers(1, 5)))]
    finally:
        fz.ODD_HEIGHTS = saved
    if len({c.shape[1] for c in clouds}) > 1:
        clouds = [np.ascontiguousarray(c[:, :3]) for c in clouds]
    return p, clouds


def assert_same_result(a, b, what):
    for fld in ("ground_idx", "nonground_idx", "ground", "nonground", "centers", "normals", "elevation_thr", "flatness_thr"):
        assert np.array_equal(getattr(a, fld), getattr(b, fld), equal_nan=True), "%s: %s differs" % (what, fld)
    assert a.sensor_height == b.sensor_height, "%s: sensor height differs" % what
    for r in range(4):
        assert np.array_equal(a.hist_elev[r], b.hist_elev[r]), "%s: elevation history of ring %d differs" % (what, r)
        assert np.array_equal(a.hist_flat[r], b.hist_flat[r]), "%s: flatness history of ring %d differs" % (what, r)


def test_restatement_equals_reference_builds_on_fuzzer_cases(oracle_built):
    refs = [(a, name, oracle_built.reference(a)) for a, name in ARITHS]
    if any(lib is None for _, _, lib in refs):
        pytest.skip("oracle/_ref not built here (needs /root/reference)")
    fz = _fuzzer()
    mine = oracle_built.restatement()
    odd_frames = 0
    for seed in SEEDS:
        p, clouds = draw_case(fz, mine, seed)
        odd_frames += sum(int(np.any(~np.isfinite(c[:, 2])) or np.any(np.abs(c[:, 2]) >= 1e30)) for c in clouds)
        for arith, name, ref in refs:
            a, b = ol.Estimator(ref, p, arith=arith), ol.Estimator(mine, p, arith=arith)
            for k, pts in enumerate(clouds):
                assert_same_result(a.run(pts), b.run(pts), "seed %d, %s, frame %d of %d" % (seed, name, k, len(clouds)))
    assert odd_frames > 0, "no seed drew the odd heights"


# ---- values at the input boundary ---------------------------------------------------------------------------------------------
F32 = np.float32
SUB = float(np.finfo(F32).smallest_subnormal)


def _r(x, y):
    """The reference's radius (xy2radius, patchworkpp.cpp:573-576): double arithmetic on the float coordinates."""
    x, y = float(F32(x)), float(F32(y))
    return math.sqrt(x * x + y * y)


def _ver_angle(x, y, z):
    """The reference's vertical angle (reflected_noise_removal, patchworkpp.cpp:387-389), in its order of operations."""
    return math.atan2(float(F32(z)), _r(x, y)) * 180 / math.pi


def boundary_case(lib, kind, seed=41):
    """(params, cloud): a synthetic cloud with additions at the input boundary, all with a finite z -- x or y NaN / +-inf,
    NaN intensities, +-0.0 and subnormal x / y, points whose radius is exactly min_range / max_range, RNR inputs exactly at
    RNR_intensity_thr and at RNR_ver_angle_thr.  kind "default": the default Params, the boundaries at their float neighbours
    (2.7, 0.2 and -15 have none on the float grid); kind "ties": min_range, RNR_intensity_thr and RNR_ver_angle_thr moved onto
    values the float inputs reach exactly."""
    p = lib.default_params()
    nan, inf = float("nan"), float("inf")
    low = -3.5  # below -sensor_height - 0.8: RNR applies where the angle and the intensity say so
    add = []
    for v in (nan, inf, -inf):
        add += [[v, 5.0, -1.7, 0.5], [5.0, v, -1.7, 0.5], [v, v, -1.7, 0.5], [v, -v, 0.3, 0.5], [v, 3.0, low, 0.05], [-4.0, v, low, 0.5]]
    add += [[4.0, 1.0, low, nan], [10.0, 2.0, -1.7, nan], [-7.0, 3.0, low, nan], [30.0, -1.0, -1.6, nan]]
    for a in (0.0, -0.0, SUB, -SUB, 1e-40, -1e-40, F32(np.finfo(F32).tiny)):
        add += [[a, 10.0, -1.7, 0.5], [10.0, a, -1.7, 0.5], [-10.0, a, -1.7, 0.5], [a, -20.0, -1.6, 0.5], [a, a, -1.7, 0.5],
                [-a, 6.0, low, 0.05]]
    f27 = F32(2.7)
    if kind == "ties":
        p.min_range = float(f27)  # = the radius of (2.7f, 0): the float input lands on it exactly
        p.RNR_intensity_thr = 0.25
        tie = (6.0, 0.0, low)
        p.RNR_ver_angle_thr = _ver_angle(*tie)
        steeper = (6.0, 0.0, float(np.nextafter(F32(low), F32(-inf))))
        assert _ver_angle(*steeper) < p.RNR_ver_angle_thr
        add += [[*tie, 0.1], [*tie, 0.1], [*steeper, 0.1], [*tie, 0.0], [0.0, 6.0, low, 0.1]]
        assert _ver_angle(0.0, 6.0, low) == p.RNR_ver_angle_thr  # (same radius on the other axis)
    mn, mx = p.min_range, p.max_range
    below, above = float(np.nextafter(F32(mn), F32(0))), float(np.nextafter(F32(mn), F32(inf)))
    for rr in (float(f27), below, above):
        add += [[rr, 0.0, -1.7, 0.5], [0.0, -rr, -1.7, 0.5], [-rr, 0.0, -1.65, 0.5], [0.0, rr, -1.75, 0.5]]
    for x, y in ((80.0, 0.0), (48.0, 64.0), (-64.0, 48.0), (0.0, -80.0), (-48.0, -64.0)):
        assert _r(x, y) == mx == 80.0
        add += [[x, y, -1.7, 0.5], [x, y, -1.2, 0.5]]
    add += [[float(np.nextafter(F32(80.0), F32(inf))), 0.0, -1.7, 0.5], [0.0, float(np.nextafter(F32(-80.0), F32(-inf))), -1.7, 0.5]]
    assert sum(_r(x, y) == mn for x, y, _, _ in add) >= (4 if kind == "ties" else 0)
    # the intensity threshold: exactly on it (not below: kept), one float below (removed); the same with the default 0.2
    thr = F32(p.RNR_intensity_thr)
    assert float(np.nextafter(thr, F32(0))) < p.RNR_intensity_thr <= float(thr)
    assert kind != "ties" or float(thr) == p.RNR_intensity_thr
    for i in (thr, np.nextafter(thr, F32(0)), np.nextafter(thr, F32(1))):
        add += [[5.0, 0.0, low, float(i)], [-3.0, -4.0, low, float(i)]]
    pts = pwpp_synth.make_cloud(seed, beams=32, azimuth_steps=900)
    extra = np.asarray(add, np.float32)
    assert np.isfinite(extra[:, 2]).all()  # (a NaN height is undefined in the reference: it sorts bins with a.z < b.z)
    rng = np.random.default_rng(seed)
    out = np.concatenate([pts, extra, extra[:, [1, 0, 2, 3]]])  # (and every addition mirrored: x and y swapped)
    rng.shuffle(out, axis=0)
    return p, np.ascontiguousarray(out)


@pytest.mark.parametrize("kind", ["default", "ties"])
def test_boundary_values_restatement_equals_reference_builds(oracle_built, kind):
    refs = [(a, name, oracle_built.reference(a)) for a, name in ARITHS]
    if any(lib is None for _, _, lib in refs):
        pytest.skip("oracle/_ref not built here (needs /root/reference)")
    mine = oracle_built.restatement()
    p, pts = boundary_case(mine, kind)
    for arith, name, ref in refs:
        a, b = ol.Estimator(ref, p, arith=arith).run(pts), ol.Estimator(mine, p, arith=arith).run(pts)
        assert_same_result(a, b, "%s, %s" % (kind, name))
