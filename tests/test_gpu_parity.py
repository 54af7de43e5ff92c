"""Parity of the HIP path (through the C-ABI, libpwpp_hip.so) with the CPU oracle, on a real
MI355X.  Bar (BASELINE.json north_star): integer index sets bit-exact; plane normals and
elevations within 1e-4 of the reference CPU path.  What is actually enforced is stronger:

* against oracle/pwpp_oracle.cpp in its fxp flavour (the arithmetic contract of DESIGN.md
  section 4) EVERYTHING is bit-identical: index sets, per-patch mean / normal / singular values /
  d, GLE decisions, adaptive thresholds and histories;
* against the reference's own patchworkpp.cpp (golden fixtures generated from oracle/_ref,
  eigen-f32 flavour): identical index sets on the six KITTI frames, normals/centres < 1e-4.
"""
import os

import numpy as np
import pytest

import oracle_lib as ol
import pwpp_hip
import pwpp_synth
from conftest import ground_mask

pytestmark = pytest.mark.gpu

NORMAL_TOL = 1e-4  # BASELINE.json: "plane normals/elevations within 1e-4"


@pytest.fixture(scope="module")
def oracle(oracle_built):
    return oracle_built.restatement()


def to_oracle_params(p):
    o = ol.Params()
    for name, _ in ol.Params._fields_:
        v = getattr(p, name)
        if hasattr(v, "__len__"):
            for k in range(4):
                getattr(o, name)[k] = v[k]
        else:
            setattr(o, name, v)
    return o


def assert_frame_equal(h, frame, ref, n_points, state_index=None, check_state=True):
    ng, nn, npatch = h.counts(frame)
    assert (ng, nn, npatch) == (len(ref.ground_idx), len(ref.nonground_idx), len(ref.centers))
    g = np.sort(h.ground_indices(frame))
    n = np.sort(h.nonground_indices(frame))
    assert np.array_equal(g, np.sort(ref.ground_idx)), "ground index set differs"
    assert np.array_equal(n, np.sort(ref.nonground_idx)), "non-ground index set differs"
    assert len(np.intersect1d(g, n)) == 0
    rec = h.patch_records(frame)
    assert len(rec) == len(ref.records)
    for fld in ("bin", "concentric_idx", "n_points", "n_ground", "n_nonground", "decision", "mean", "normal", "sv", "d"):
        assert np.array_equal(rec[fld], ref.records[fld], equal_nan=True), "patch field %s differs" % fld
    assert np.array_equal(h.centers(frame), ref.centers, equal_nan=True)
    assert np.array_equal(h.normals(frame), ref.normals, equal_nan=True)
    if check_state:
        st = h.state(frame if state_index is None else state_index)
        assert st.sensor_height == ref.sensor_height
        assert list(st.elevation_thr) == list(ref.elevation_thr)
        assert list(st.flatness_thr) == list(ref.flatness_thr)
        idx = frame if state_index is None else state_index
        for ring in range(4):
            assert np.array_equal(h.history(idx, 0, ring), ref.hist_elev[ring])
            assert np.array_equal(h.history(idx, 1, ring), ref.hist_flat[ring])


def reference_consensus(op, pts):
    """The ground set the three builds of the reference (oracle/_ref: float sums, exact-f64 sums, 4-lane float sums) agree
    on for one fresh frame -- None where they differ among themselves or did not travel."""
    sets = []
    for a in (ol.ARITH_EIGEN_F32, ol.ARITH_EXACT_F64, ol.ARITH_F32_PACKET4):
        lib = ol.reference(a)
        if lib is None:
            return None
        sets.append(np.sort(ol.Estimator(lib, op, arith=a).run(pts).ground_idx))
    return sets[0] if all(np.array_equal(sets[0], x) for x in sets[1:]) else None


def test_kitti_fresh_bitwise_vs_fxp_oracle(kitti, oracle):
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    for k, pts in enumerate(kitti):
        ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
        assert_frame_equal(h, k, ref, pts.shape[0])


def test_kitti_fresh_vs_reference_golden(kitti, golden):
    """IoU == 1.0 against the reference's own code (eigen-f32 flavour), normals within 1e-4."""
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    for k, pts in enumerate(kitti):
        key = "f32/fresh/%d/" % k
        mask = np.packbits(ground_mask(h.ground_indices(k), pts.shape[0]))
        assert np.array_equal(mask, golden[key + "ground_mask"])  # IoU == 1.0
        assert list(h.counts(k)) == list(golden[key + "counts"])
        assert np.abs(h.normals(k) - golden[key + "normals"]).max() < NORMAL_TOL
        assert np.abs(h.centers(k) - golden[key + "centers"]).max() < NORMAL_TOL
        st = h.state(k)
        assert abs(st.sensor_height - golden[key + "state"][0]) < NORMAL_TOL


def test_kitti_sequence_stateful(kitti, oracle, golden):
    """One long-lived object over frames 0..5 twice (demo_sequential semantics)."""
    h = pwpp_hip.Handle()
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for rep in range(2):
        for k, pts in enumerate(kitti):
            h.estimate_ground(pts)
            ref = est.run(pts)
            assert_frame_equal(h, 0, ref, pts.shape[0], state_index=0)
            assert h.height() == ref.sensor_height
            if rep == 0:
                mask = np.packbits(ground_mask(h.ground_indices(0), pts.shape[0]))
                assert np.array_equal(mask, golden["f32/seq/%d/ground_mask" % k])


def test_multi_stream_lockstep(kitti, oracle):
    """S independent streams stepped together: stream s sees frames s, s+1, ... (mod 6)."""
    S = 4
    h = pwpp_hip.Handle()
    h.set_num_streams(S)
    ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(S)]
    for t in range(4):
        frames = [kitti[(s + t) % 6] for s in range(S)]
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
        for s in range(S):
            assert_frame_equal(h, s, ests[s].run(frames[s]), frames[s].shape[0], state_index=s)


def test_multi_stream_one_pass_with_state_restore(kitti, oracle):
    """Six stateful streams in lock-step take the one-pass binning.  In step 1 one stream gets a cloud
    that overflows its bin segments: the batch is redone on the two-pass path FROM THE STATE BEFORE
    THE STEP (the first attempt had already advanced sensor height, thresholds and histories of every
    stream).  Every stream must keep following its own sequential oracle."""
    S = 6
    rng = np.random.default_rng(9)
    wedge = kitti[2].copy()
    sel = rng.random(wedge.shape[0]) < 0.7
    r = np.hypot(wedge[sel, 0], wedge[sel, 1])
    a = rng.uniform(0.1, 0.27, sel.sum())
    wedge[sel, 0] = (r * np.cos(a)).astype(np.float32)
    wedge[sel, 1] = (r * np.sin(a)).astype(np.float32)
    h = pwpp_hip.Handle()
    h.set_num_streams(S)
    ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(S)]
    redone = []
    for t in range(12):
        frames = [kitti[(s + t) % 6] for s in range(S)]
        if t == 1:
            frames[3] = wedge
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
        for s in range(S):
            assert_frame_equal(h, s, ests[s].run(frames[s]), frames[s].shape[0], state_index=s)
        redone.append(h.one_pass_stats())
    # (the redo's exact counts size the segments of the following batches: one-pass again, and nothing more is redone)
    assert redone[0] == (1, 0) and redone[1] == (2, 1) and redone[2] == (3, 1) and redone[11] == (12, 1)
    assert h.redo_stats() == (12 * S, 1)  # only stream 3 went back to its state before step 1 and was redone


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_synthetic_with_edge_cases(oracle, seed):
    pts = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(seed), seed)
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([pts], mode=pwpp_hip.MODE_FRESH)
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
    assert_frame_equal(h, 0, ref, pts.shape[0])
    ng, nn, _ = h.counts(0)
    assert ng + nn == pts.shape[0] - 1  # the z == FLT_MIN point is in neither list (ref :591)


PARAM_VARIANTS = [
    dict(enable_RNR=0), dict(enable_RVPF=0), dict(enable_TGR=0), dict(num_min_pts=0),
    dict(num_iter=1), dict(num_iter=5), dict(num_lpr=1), dict(num_lpr=64), dict(num_lpr=128), dict(num_lpr=256, num_min_pts=300), dict(num_min_pts=1), dict(num_min_pts=200),
    dict(th_dist=0.2, th_seeds=0.3), dict(uprightness_thr=0.9), dict(max_range=50.0, min_range=1.0),
    dict(sensor_height=2.0), dict(num_rings_of_interest=2), dict(adaptive_seed_selection_margin=-0.9),
    dict(sectors=(36, 36, 36, 36)), dict(sectors=(8, 8, 8, 8), rings=(1, 1, 1, 1)), dict(rings=(3, 5, 2, 6)),
    dict(elev=(-1.5, -1.4, -1.3, -1.2), flat=(1e-4, 2e-4, 3e-4, 4e-4)),
    # the dual seed pass of the big-bin kernel: R-VPF threshold below / equal to / above the R-GPF one,
    # and planes that come out vertical almost always (strip -> the stashed seed totals are dropped)
    dict(th_seeds_v=0.05), dict(th_seeds=0.25, th_seeds_v=0.25), dict(th_seeds_v=0.6, th_seeds=0.05),
    dict(uprightness_thr=0.9999, th_dist_v=0.3), dict(uprightness_thr=0.9999, th_dist_v=0.02, num_iter=2),
    # the edges of what pwpp_create accepts (tools/param_extremes.py has more)
    dict(sectors=(128, 128, 128, 128), rings=(4, 4, 4, 4)),   # 2048 bins
    dict(sectors=(1, 1, 1, 1), rings=(1, 1, 1, 1)),           # 4 bins of 10-80 k points: the workgroup kernel
    dict(max_range=200.0, min_range=0.3),                     # fixed-point shift 15
    dict(max_range=20.0, min_range=5.0),                      # most points out of range
    dict(num_lpr=64, num_iter=7, th_seeds=0.02, th_dist=0.02), dict(num_min_pts=5000), dict(uprightness_thr=1.0),
    dict(RNR_ver_angle_thr=10.0, RNR_intensity_thr=2.0),      # RNR takes almost everything below the sensor
]


def apply_variant(p, variant):
    for k, v in variant.items():
        if k == "sectors":
            for i in range(4):
                p.num_sectors_each_zone[i] = v[i]
        elif k == "rings":
            for i in range(4):
                p.num_rings_each_zone[i] = v[i]
        elif k == "elev":
            for i in range(4):
                p.elevation_thr[i] = v[i]
        elif k == "flat":
            for i in range(4):
                p.flatness_thr[i] = v[i]
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("variant", PARAM_VARIANTS, ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()))
def test_parameter_variants(kitti, oracle, variant):
    p = apply_variant(pwpp_hip.default_params(), variant)
    h = pwpp_hip.Handle(p)
    est = ol.Estimator(oracle, to_oracle_params(p), arith=ol.ARITH_FXP)
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(5, beams=48, azimuth_steps=1500), 5)
    tiny_prone = variant.get("num_min_pts", 10) < 4 or variant.get("num_lpr", 20) < 4
    for k, pts in enumerate((kitti[0], syn, kitti[4])):
        h.estimate_ground(pts)
        assert_frame_equal(h, 0, est.run(pts), pts.shape[0], state_index=0)
        if tiny_prone and k == 0:
            # fit sets of 1-3 points follow the reference's own float arithmetic (contract v3): IoU == 1.0 against the REFERENCE
            # BUILD wherever its three flavours agree (fresh object: the first frame of the sequence)
            want = reference_consensus(to_oracle_params(p), pts)
            if want is not None:
                assert np.array_equal(np.sort(h.ground_indices(0)), want), "ground set differs from the reference build"
    # the same frames as one batch (one-pass binning), under the plan the launcher picks for this
    # little work (one wave per patch) and under the plans of bigger batches (k_fit_w64 kernels)
    frames = [kitti[1], syn, kitti[3], kitti[0], kitti[5], syn]
    refs = [ol.Estimator(oracle, to_oracle_params(p), arith=ol.ARITH_FXP).run(pts) for pts in frames]
    hb = pwpp_hip.Handle(p)
    for plan in ("", "W16:1023,W64.2:65535", "W16.16:1023,S64:65535"):
        hb.set_option("fit_plan", plan)
        hb.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        for i, pts in enumerate(frames):
            assert_frame_equal(hb, i, refs[i], pts.shape[0])


def test_layouts_and_three_columns(kitti, oracle):
    p = pwpp_hip.default_params()
    p.enable_RNR = 0
    pts = kitti[2]
    ref = ol.Estimator(oracle, to_oracle_params(p), arith=ol.ARITH_FXP).run(pts)
    for arr in (pts, np.asfortranarray(pts), pts[:, :3].copy(), np.asfortranarray(pts[:, :3])):
        h = pwpp_hip.Handle(p)
        h.estimate_ground(arr)
        assert_frame_equal(h, 0, ref, pts.shape[0], state_index=0)
    # the same layouts as batches (one-pass binning reads them through the same accessor)
    refs = [ol.Estimator(oracle, to_oracle_params(p), arith=ol.ARITH_FXP).run(k) for k in kitti]
    hb = pwpp_hip.Handle(p)
    for conv in (lambda k: np.ascontiguousarray(k[:, :3]), np.asfortranarray, lambda k: np.asfortranarray(k[:, :3])):
        hb.estimate_ground_batch([conv(k) for k in kitti], mode=pwpp_hip.MODE_FRESH)
        for i in range(6):
            assert_frame_equal(hb, i, refs[i], kitti[i].shape[0])
    # with RNR on, a 3-column cloud skips RNR (ref :379-382) but must still work
    h = pwpp_hip.Handle()
    h.estimate_ground(pts[:, :3].copy())
    ref3 = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts[:, :3].copy())
    assert_frame_equal(h, 0, ref3, pts.shape[0], state_index=0)


def test_xyz_getters_align_with_indices(kitti):
    h = pwpp_hip.Handle()
    h.estimate_ground(kitti[3])
    assert np.array_equal(h.ground(), kitti[3][h.ground_indices(), :3])
    assert np.array_equal(h.nonground(), kitti[3][h.nonground_indices(), :3])


def test_ragged_and_degenerate_frames(oracle):
    rng = np.random.default_rng(0)
    base = pwpp_synth.make_cloud(9, beams=16, azimuth_steps=500)
    frames = [
        base, base[:1], base[:9], base[:10], base[:11], np.zeros((0, 4), np.float32),
        np.tile(np.array([[10.0, 3.0, -1.7, 0.5]], np.float32), (500, 1)),           # 500 identical points
        np.concatenate([base[:3000], np.full((5, 4), np.nan, np.float32)]),             # NaN rows -> out of range
        (base[:2000] * np.array([1, 1, 0, 1], np.float32)),                             # all z == 0
        np.concatenate([np.array([[6.0, 2.0, -9.0, 0.9]], np.float32), base[:4000]]),   # one deep outlier
        rng.uniform(-90, 90, (5000, 4)).astype(np.float32),                             # noise
    ]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for k, pts in enumerate(frames):
        ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts) if len(pts) else None
        if ref is None:
            assert h.counts(k) == (0, 0, 0)
            continue
        assert_frame_equal(h, k, ref, pts.shape[0])


def test_dense_128_beam_cloud_36_sectors(oracle):
    """BASELINE.json configs[4]: ~500k-point cloud, 36-sector CZM (bins far beyond LDS size)."""
    p = pwpp_hip.default_params()
    for i in range(4):
        p.num_sectors_each_zone[i] = 36
    pts = pwpp_synth.make_dense_cloud(3)
    assert pts.shape[0] > 400000
    h = pwpp_hip.Handle(p)
    h.estimate_ground(pts)
    ref = ol.Estimator(oracle, to_oracle_params(p), arith=ol.ARITH_FXP).run(pts)
    assert_frame_equal(h, 0, ref, pts.shape[0], state_index=0)
    h2 = pwpp_hip.Handle()  # default 16 zone-0 sectors: ~30k-point bins
    h2.estimate_ground(pts)
    ref2 = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
    assert_frame_equal(h2, 0, ref2, pts.shape[0], state_index=0)


def test_large_batch_properties(kitti, oracle):
    """256 frames in one launch set (the mid-size plans, two frame ranges): replays agree with each other and with
    the oracle, every frame is partitioned."""
    F = 256
    frames = [kitti[i % 6] for i in range(F)]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    counts = h.all_counts()
    for i in range(F):
        assert tuple(counts[i, :3]) == tuple(counts[i % 6, :3])
        assert counts[i, 0] + counts[i, 1] + counts[i, 5] == frames[i].shape[0]
    for i in (6, 100, 255):
        assert np.array_equal(np.sort(h.ground_indices(i)), np.sort(h.ground_indices(i % 6)))
        assert np.array_equal(h.normals(i), h.normals(i % 6))
    g = h.ground_indices(255)
    n = h.nonground_indices(255)
    assert np.array_equal(np.sort(np.concatenate([g, n])), np.arange(frames[255].shape[0]))
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(k) for k in kitti]
    for i in (0, 7, 127, 128, 200, 255):
        assert_frame_equal(h, i, refs[i % 6], frames[i].shape[0])


def test_pybind_module_end_to_end(kitti, golden):
    import pypatchworkpp
    params = pypatchworkpp.Parameters()
    pw = pypatchworkpp.patchworkpp(params)
    for k in range(3):
        pw.estimateGround(kitti[k])
        gi = pw.getGroundIndices()
        assert gi.dtype == np.int32 and pw.getGround().shape == (len(gi), 3)
        mask = np.packbits(ground_mask(gi, kitti[k].shape[0]))
        assert np.array_equal(mask, golden["f32/seq/%d/ground_mask" % k])
        assert np.array_equal(pw.getGround(), kitti[k][gi, :3])
        assert len(gi) + len(pw.getNongroundIndices()) == kitti[k].shape[0]
        assert pw.getCenters().shape == pw.getNormals().shape
        assert abs(pw.getHeight() - golden["f32/seq/%d/state" % k][0]) < 1e-4
        assert pw.getTimeTaken() > 0
    pw.estimateGround(np.asfortranarray(kitti[0]).astype(np.float64))  # any array convertible to float32
    # extension: the reference's own order inside a patch's part of the lists (z-sorted bins)
    pw2 = pypatchworkpp.patchworkpp(params)
    pw2.setReferenceOrder(True)
    pw2.estimateGround(kitti[3])
    h = pwpp_hip.Handle()
    h.set_output_order(True)
    h.estimate_ground_batch([kitti[3]], mode=pwpp_hip.MODE_STREAMS)
    assert np.array_equal(pw2.getGroundIndices(), h.ground_indices(0))
    assert np.array_equal(pw2.getNonground(), kitti[3][h.nonground_indices(0), :3])


def test_points_on_bin_boundaries(oracle):
    """The float fast path of the CZM binning must hand every point near a ring / sector / zone /
    range boundary to the exact double computation: clouds made of points within a few float
    ulps of the boundaries, compared bin by bin (patch point counts) with the oracle."""
    rng = np.random.default_rng(42)
    p = pwpp_hip.default_params()
    mn, mx = p.min_range, p.max_range
    z2, z3, z4 = (7 * mn + mx) / 8.0, (3 * mn + mx) / 4.0, (mn + mx) / 2.0
    mins = [mn, z2, z3, z4, mx]
    radii = []
    for k in range(4):
        for r in range(p.num_rings_each_zone[k] + 1):
            radii.append(mins[k] + (mins[k + 1] - mins[k]) * r / p.num_rings_each_zone[k])
    radii = np.array(radii)
    pts = []
    for k in range(4):
        ns = p.num_sectors_each_zone[k]
        for s in range(ns + 1):
            th = 2 * np.pi * s / ns
            for r in rng.uniform(mins[k], mins[k + 1], 40):
                for d in (-3e-7, -1e-7, 0.0, 1e-7, 3e-7):
                    pts.append([r * np.cos(th + d), r * np.sin(th + d)])
    for r in radii:
        for th in rng.uniform(0, 2 * np.pi, 60):
            for d in (-2e-6, -5e-7, 0.0, 5e-7, 2e-6):
                pts.append([(r * (1 + d)) * np.cos(th), (r * (1 + d)) * np.sin(th)])
    xy = np.array(pts)
    cloud = np.zeros((len(xy), 4), np.float32)
    cloud[:, :2] = xy
    cloud[:, 2] = -1.7 + rng.normal(0, 0.03, len(xy))
    cloud[:, 3] = 0.5
    filler = pwpp_synth.make_cloud(21, beams=32, azimuth_steps=1200)
    cloud = np.concatenate([cloud, filler])
    h = pwpp_hip.Handle()
    h.estimate_ground(cloud)
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(cloud)
    assert_frame_equal(h, 0, ref, cloud.shape[0], state_index=0)


@pytest.mark.parametrize("plan", ["S8:63,S16:255,S32:1023,S64:4095", "S8:65535", "S64:65535", "W16:65535", "S16:100",
                                  "W16.16:1023,W64.2:65535", "W16.32:511,W64.4:65535", "W16:255,W64.8:65535", "S64:255,B64:65535",
                                  "B64:65535", "H64:511", "H64:63"])
def test_every_fit_kernel_variant(kitti, oracle, plan):
    """All fit kernels (streaming rows of every width, 16 / 32 / 64 small patches per wave, 2 / 4 / 8 big bins per
    wave, four waves per patch, the workgroup kernel for whatever exceeds the plan) produce the same bit-exact
    result: the integer plane-fit sums do not depend on how many lanes share a patch."""
    h = pwpp_hip.Handle()
    h.set_option("fit_plan", plan)
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(8), 8)
    h.estimate_ground_batch([kitti[0], syn, kitti[5]], mode=pwpp_hip.MODE_FRESH)
    for k, pts in enumerate((kitti[0], syn, kitti[5])):
        assert_frame_equal(h, k, ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts), pts.shape[0])


_SPLIT_REFS = {}


@pytest.mark.parametrize("zones", [1, 4])
@pytest.mark.parametrize("hi_split", [-1.0, 0.0, 0.05, 0.6, 3.0, 1e30])
def test_results_do_not_depend_on_where_the_bins_are_split(kitti, oracle, hi_split, zones):
    """A bin is stored in two parts (below / at or above a split height) and the fit passes skip the high part whenever
    they can prove it irrelevant (pwpp_fit.hip, stage_needs_hi).  Wherever the split lies -- below nearly every point
    (the lowest-point selection must then go on into the high part, every seed pass needs it), at the ground, far
    above everything, in the near zone only or in every bin -- and whichever kernel fits the patch, the result is
    the oracle's, bit for bit.  The synthetic frame adds walls next to the sensor (R-VPF strips points of both
    parts), +-inf heights and steep ground in the near zone."""
    rng = np.random.default_rng(99)
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(31, n_boxes=80, undulation=0.6), 31)
    wall = np.zeros((6000, 4), np.float32)   # vertical walls 4-9 m from the sensor, from below the ground to 2 m above
    wall[:, 0] = rng.uniform(4.0, 9.0, 6000)
    wall[:, 1] = np.repeat(rng.uniform(-6.0, 6.0, 12), 500) + rng.normal(0, 0.01, 6000)
    wall[:, 2] = rng.uniform(-2.2, 0.4, 6000)
    wall[:, 3] = 0.5
    odd = np.array([[5.0, 2.0, np.inf, 0.5], [5.1, 2.0, -np.inf, 0.5], [-6.0, 3.0, np.inf, 0.5], [7.0, -2.5, 1e30, 0.5],
                    [7.0, -2.6, -1e30, 0.5]], np.float32)
    syn = np.concatenate([syn, wall, odd]).astype(np.float32)
    frames = [kitti[0], syn, kitti[5]]
    if not _SPLIT_REFS:
        for k, pts in enumerate(frames):
            _SPLIT_REFS[k] = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts)
    for plan in ("", "W16:1023,W64.2:65535", "S16:255,S64:65535", "B64:65535", "S16:100"):
        h = pwpp_hip.Handle()
        h.set_option("hi_split", hi_split)
        h.set_option("hi_split_zones", zones)
        if plan:
            h.set_option("fit_plan", plan)
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        for k, pts in enumerate(frames):
            assert_frame_equal(h, k, _SPLIT_REFS[k], pts.shape[0])


def test_split_bins_in_reference_order_and_one_pass_batches(kitti, oracle):
    """The two list modes and the two binning paths with split bins: reference order (the R-VPF round of a removed point
    of a skipped high part comes from the part itself, k_emit), and a one-pass batch whose segments were sized for
    another split (overflow, exact redo)."""
    frames = [kitti[k % 6] for k in range(12)]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(kitti[k]) for k in range(6)]
    for order in (False, True):
        h = pwpp_hip.Handle()
        h.set_output_order(order)
        for hi_split in (0.6, 0.0, 2.0):
            h.set_option("hi_split", hi_split)
            h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
            for k in range(12):
                assert_frame_equal(h, k, refs[k % 6], kitti[k % 6].shape[0])
                if order:  # the reference's own order of the lists (ties aside: the z sequence)
                    z = kitti[k % 6][:, 2]
                    assert np.array_equal(z[h.ground_indices(k)], z[refs[k % 6].ground_idx])
                    assert np.array_equal(z[h.nonground_indices(k)], z[refs[k % 6].nonground_idx])


def test_randomised_differential_cases(oracle):
    """tools/fuzz_parity.py: random parameter sets, random clouds with walls / ramps / huge and infinite heights /
    duplicates, random bin splits and fit plans, fresh batches, stateful sequences and lock-step streams -- every case
    bit-identical to the oracle (3 200 more seeds ran clean when this was written; a failing seed reproduces with
    `python tools/fuzz_parity.py 1 <seed>`)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    for seed in range(5000, 5040):
        fz.one_case(seed, oracle)


def test_ingest_pinned_buffers_and_bulk_index_copy(kitti):
    """frames handed over in page-locked buffers, every index list of the batch
    fetched with one device-to-host copy; same content as the per-frame getters."""
    frames = []
    for k in range(4):
        a = pwpp_hip.pinned_empty(kitti[k].shape)
        a[:] = kitti[k]
        frames.append(a)
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    out = pwpp_hip.pinned_empty((sum(f.shape[0] for f in frames),), np.int32)
    idx, base, counts = h.all_indices(out)
    assert base[-1] == sum(f.shape[0] for f in frames)
    for k in range(4):
        ng, nn = counts[k, 0], counts[k, 1]
        assert (ng, nn) == h.counts(k)[:2]
        assert np.array_equal(idx[base[k]:base[k] + ng], h.ground_indices(k))
        assert np.array_equal(idx[base[k] + ng:base[k] + ng + nn], h.nonground_indices(k))
    for a in frames:
        pwpp_hip.pinned_free(a)
    pwpp_hip.pinned_free(out)


def test_ingest_async_pinned_slab_two_handles(kitti, oracle):
    """PWPP_MEM_HOST_PINNED is asynchronous; frames that lie back to back in one
    page-locked slab go over in merged copies; two handles (= two streams) work on two chunks at once.
    Results are the oracle's."""
    chunks = [[0, 1, 2, 3, 4, 5, 0], [5, 4, 3, 2, 1]]   # 7 frames: one-pass binning; 5 frames too
    slabs, views = [], []
    for ids in chunks:
        rows = sum(kitti[k].shape[0] for k in ids)
        slab = pwpp_hip.pinned_empty((rows, 4))
        at, fr = 0, []
        for k in ids:
            n = kitti[k].shape[0]
            slab[at:at + n] = kitti[k]
            fr.append(slab[at:at + n])
            at += n
        slabs.append(slab)
        views.append(fr)
    ha, hb = pwpp_hip.Handle(), pwpp_hip.Handle()
    ha.submit_pinned_batch(views[0])   # returns at once
    hb.submit_pinned_batch(views[1])
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(kitti[k]) for k in range(6)]
    for h, ids in ((ha, chunks[0]), (hb, chunks[1])):
        h.synchronize()
        for i, k in enumerate(ids):
            assert_frame_equal(h, i, refs[k], kitti[k].shape[0])
    for s_ in slabs:
        pwpp_hip.pinned_free(s_)


def test_cpp_class_demo_program(kitti, golden, tmp_path):
    """The C++ mirror of patchwork::PatchWorkpp through a compiled program that follows the
    reference's demo_sequential.cpp: one object over frames 0..2, counts and sensor height as the
    reference produces them (golden: reference build, sequence mode)."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "patchwork-plusplus_amd", "examples", "demo_sequential")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "patchwork-plusplus_amd"), "examples/demo_sequential"], check=True)
    paths = []
    for k in range(3):
        p = tmp_path / ("%06d.bin" % k)
        kitti[k].tofile(p)
        paths.append(str(p))
    out = subprocess.run([exe] + paths, capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.splitlines() if "Ground Points" in l]
    assert len(lines) == 3, out
    for k, line in enumerate(lines):
        ng = int(re.search(r"Ground Points #: (\d+)", line).group(1))
        nn = int(re.search(r"Nonground Points #: (\d+)", line).group(1))
        npat = int(re.search(r"patches: (\d+)", line).group(1))
        height = float(re.search(r"height: ([-0-9.]+)", line).group(1))
        assert [ng, nn, npat] == list(golden["f32/seq/%d/counts" % k])
        assert abs(height - golden["f32/seq/%d/state" % k][0]) < 1e-4


def test_c_abi_demo_program(kitti, golden, tmp_path):
    """The C-ABI driven from plain C99 (examples/capi_demo.c): a fresh handle on frame 0 gives the reference's
    counts (golden: reference build, fresh state)."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "patchwork-plusplus_amd", "examples", "capi_demo")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "patchwork-plusplus_amd"), "examples/capi_demo"], check=True)
    p = tmp_path / "000000.bin"
    kitti[0].tofile(p)
    out = subprocess.run([exe, str(p)], capture_output=True, text=True, check=True).stdout
    m = re.search(r"points (\d+) ground (\d+) nonground (\d+) patches (\d+) height ([-0-9.]+)", out)
    assert m, out
    assert int(m.group(1)) == kitti[0].shape[0]
    assert [int(m.group(2)), int(m.group(3)), int(m.group(4))] == list(golden["f32/seq/0/counts"])
    assert abs(float(m.group(5)) - golden["f32/seq/0/state"][0]) < 1e-4
    assert "pipe depth 2: 4 batches of 3 frames, every frame equal to the single call" in out  # (pwpp_pipe_* from C)
    assert re.search(r"pipe in stream mode: 2 groups of 2 streams, 3 steps each, every stream at one handle's sensor height", out), out


def test_one_pass_binning_and_its_overflow_fallback(kitti, oracle):
    """Batches of independent frames bin in one pass into fixed bin segments (k_czm_bin_scatter).
    The segments are sized from the bins' largest counts so far (1.5 x + 256 slots; before the first batch from
    a histogram of sample frames).
    (1) KITTI frames: the one-pass path is taken and nothing is redone;
    (3) a cloud with most points in one sector overflows segments sized for KITTI frames: the batch is redone
        on the exact two-pass path, whose counts then size the segments -- the same cloud fits afterwards;
    (2) with absurdly small segments every frame overflows, same fallback; results are the oracle's either way."""
    frames = [kitti[i % 6] for i in range(7)]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p) for p in frames[:6]]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for i, pts in enumerate(frames):
        assert_frame_equal(h, i, refs[i % 6], pts.shape[0])
    assert h.one_pass_stats() == (1, 0)
    # (3) 70 % of a frame's points squeezed into a 10-degree wedge (still a valid cloud)
    rng = np.random.default_rng(5)
    wedge = kitti[0].copy()
    sel = rng.random(wedge.shape[0]) < 0.7
    r = np.hypot(wedge[sel, 0], wedge[sel, 1])
    a = rng.uniform(0.1, 0.27, sel.sum())
    wedge[sel, 0] = (r * np.cos(a)).astype(np.float32)
    wedge[sel, 1] = (r * np.sin(a)).astype(np.float32)
    odd = [wedge, kitti[1], kitti[2], wedge, kitti[3]]
    h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
    for i, pts in enumerate(odd):
        assert_frame_equal(h, i, ol.Estimator(oracle, arith=ol.ARITH_FXP).run(pts), pts.shape[0])
    assert h.one_pass_stats() == (2, 1)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for i, pts in enumerate(frames):
        assert_frame_equal(h, i, refs[i % 6], pts.shape[0])
    assert h.one_pass_stats() == (3, 1)
    h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)  # the wedge fits the rebuilt segments
    for i in (0, 3, 4):
        assert_frame_equal(h, i, ol.Estimator(oracle, arith=ol.ARITH_FXP).run(odd[i]), odd[i].shape[0])
    assert h.one_pass_stats() == (4, 1)
    # (2)
    h2 = pwpp_hip.Handle()
    h2.set_option("one_pass_scale", 0.05)
    h2.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for i, pts in enumerate(frames):
        assert_frame_equal(h2, i, refs[i % 6], pts.shape[0])
    assert h2.one_pass_stats() == (1, 1)


def test_an_overflow_costs_its_frame_not_the_batch(kitti, oracle):
    """the reference's bins are unbounded vectors (patchworkpp.cpp:578-622), the one-pass binning gives
    every bin a fixed segment.  One frame of 256 overflows its segments: exactly that frame is binned again (exact
    two-pass path, in place), every one of the 256 frames is the oracle's bit for bit, fresh frames and reference-ordered
    lists alike; with the option "redo_whole_batch" (rounds 1-4) every frame counts as redone and the results are the same.
    Then three outliers, two of them neighbours (one run through the pipeline), and one at each end of the batch."""
    rng = np.random.default_rng(5)

    def wedge_of(src, lo):
        w = src.copy()
        sel = rng.random(w.shape[0]) < 0.7
        r = np.hypot(w[sel, 0], w[sel, 1])
        a = rng.uniform(lo, lo + 0.17, sel.sum())
        w[sel, 0] = (r * np.cos(a)).astype(np.float32)
        w[sel, 1] = (r * np.sin(a)).astype(np.float32)
        return w

    est = lambda p: ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p)
    refs = [est(k) for k in kitti]
    F = 256
    base = [kitti[i % 6] for i in range(F)]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(base, mode=pwpp_hip.MODE_FRESH)
    assert h.one_pass_stats() == (1, 0) and h.redo_stats() == (F, 0)
    w0 = wedge_of(kitti[0], 0.1)
    odd = list(base)
    odd[77] = w0
    h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
    assert h.one_pass_stats() == (2, 1) and h.redo_stats() == (2 * F, 1)
    rw0 = est(w0)
    for i in range(F):
        assert_frame_equal(h, i, rw0 if i == 77 else refs[i % 6], odd[i].shape[0], check_state=(i % 32 == 13))
    # the redone frame's exact counts sized the table: the same batch fits now
    h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
    assert h.redo_stats() == (3 * F, 1)
    assert_frame_equal(h, 77, rw0, w0.shape[0])
    # three outliers in other sectors: first frame, two neighbours, last frame
    w1, w2, w3 = wedge_of(kitti[1], 1.3), wedge_of(kitti[2], 2.6), wedge_of(kitti[3], -2.0)
    odd2 = list(base)
    odd2[0], odd2[100], odd2[101], odd2[F - 1] = w1, w2, w3, w1
    h.estimate_ground_batch(odd2, mode=pwpp_hip.MODE_FRESH)
    assert h.redo_stats() == (4 * F, 5)
    special = {0: est(w1), 100: est(w2), 101: est(w3), F - 1: est(w1)}
    for i in list(special) + [1, 99, 102, 128, F - 2]:
        assert_frame_equal(h, i, special.get(i, refs[i % 6]), odd2[i].shape[0])
    # rounds 1-4's behaviour behind an option: same results, every frame redone
    h2 = pwpp_hip.Handle()
    h2.set_option("redo_whole_batch", 1)
    h2.estimate_ground_batch(base, mode=pwpp_hip.MODE_FRESH)
    h2.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
    assert h2.one_pass_stats() == (2, 1) and h2.redo_stats() == (2 * F, F)
    for i in (0, 76, 77, 78, F - 1):
        assert_frame_equal(h2, i, rw0 if i == 77 else refs[i % 6], odd[i].shape[0])
    # reference-ordered lists (single-stream schedule + the sort kernels) through the same in-place redo
    h3 = pwpp_hip.Handle()
    h3.set_output_order(True)
    small = [kitti[i % 6] for i in range(12)]
    h3.estimate_ground_batch(small, mode=pwpp_hip.MODE_FRESH)
    small[5] = w0
    h3.estimate_ground_batch(small, mode=pwpp_hip.MODE_FRESH)
    assert h3.redo_stats() == (24, 1)
    for i in (4, 5, 6):
        r = rw0 if i == 5 else refs[i % 6]
        assert_frame_equal(h3, i, r, small[i].shape[0])
        assert np.array_equal(small[i][h3.ground_indices(i), 2], small[i][r.ground_idx, 2])  # same heights position by position (ties in cloud order)


def test_long_lists_in_a_big_batch(kitti, oracle):
    """k_emit in big batches (round 5): one wave per bin, and a second launch with extra waves for the bins the handle has seen more
    than 8192 entries in.  A frame with 60 % of its points closer than min_range (a pseudo-bin of ~75 k entries: bench.py's `distinct`
    leg has such frames -- a box over the sensor), one with 40 % beyond max_range, a wedge whose bins hold tens of thousands of points
    (lists compacted from the membership plane).  First batch: the bins are not in the table yet, their one wave copies everything;
    second and third batch: the table knows them.  Reference-ordered lists take the same second launch."""
    rng = np.random.default_rng(21)

    def scaled(src, frac, lo, hi):
        w = src.copy()
        sel = rng.random(w.shape[0]) < frac
        r = np.hypot(w[sel, 0], w[sel, 1])
        s = rng.uniform(lo, hi, sel.sum()) / np.maximum(r, 1e-3)
        w[sel, 0] = (w[sel, 0] * s).astype(np.float32)
        w[sel, 1] = (w[sel, 1] * s).astype(np.float32)
        return w

    near, far = scaled(kitti[1], 0.6, 0.3, 2.5), scaled(kitti[2], 0.4, 85.0, 110.0)
    wedge = kitti[0].copy()
    sel = rng.random(wedge.shape[0]) < 0.7
    r = np.hypot(wedge[sel, 0], wedge[sel, 1])
    a = rng.uniform(0.1, 0.27, sel.sum())
    wedge[sel, 0] = (r * np.cos(a)).astype(np.float32)
    wedge[sel, 1] = (r * np.sin(a)).astype(np.float32)
    est = lambda p: ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p)
    refs = [est(k) for k in kitti]
    F = 72
    frames = [kitti[i % 6] for i in range(F)]
    special = {3: near, 40: far, 41: wedge, F - 1: near}
    want = {i: est(p) for i, p in special.items()}
    for i, p in special.items():
        frames[i] = p
    assert max(len(r.nonground_idx) for r in want.values()) > 60000
    h = pwpp_hip.Handle()
    for rep in range(3):
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        for i in list(special) + [0, 2, 4, 39, 42, F - 2]:
            assert_frame_equal(h, i, want.get(i, refs[i % 6]), frames[i].shape[0], check_state=(rep == 0))
    h.set_output_order(True)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for i in (3, 41, 42):
        r = want.get(i, refs[i % 6])
        assert np.array_equal(frames[i][h.ground_indices(i), 2], frames[i][np.asarray(r.ground_idx), 2])
        assert np.array_equal(np.sort(h.nonground_indices(i)), np.sort(r.nonground_idx))


def test_point_order_invariance_and_determinism(kitti):
    """Size-independent properties of the arithmetic contract: the plane-fit sums
    are exact integers, so (1) shuffling the rows of a cloud gives the same ground SET (indices mapped
    back), bit-identical patch planes and the same adaptive state; (2) two runs of the same batch give
    identical outputs although the scatter order inside a bin depends on atomics."""
    rng = np.random.default_rng(11)
    frames, perms = [], []
    for k in range(6):
        perm = rng.permutation(kitti[k].shape[0])
        frames += [kitti[k], np.ascontiguousarray(kitti[k][perm])]
        perms.append(perm)
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    first = [(np.sort(h.ground_indices(i)), h.normals(i).copy(), h.centers(i).copy(), h.patch_records(i).copy()) for i in range(12)]
    for k in range(6):
        g0, nrm0, ctr0, rec0 = first[2 * k]
        g1, nrm1, ctr1, rec1 = first[2 * k + 1]
        assert np.array_equal(g0, np.sort(perms[k][g1])), "ground set changed under a permutation of the input rows"
        assert np.array_equal(nrm0, nrm1, equal_nan=True) and np.array_equal(ctr0, ctr1, equal_nan=True)
        for fld in ("n_points", "n_ground", "decision", "sv", "d"):
            assert np.array_equal(rec0[fld], rec1[fld], equal_nan=True)
        s0, s1 = h.state(2 * k), h.state(2 * k + 1)
        assert s0.sensor_height == s1.sensor_height and list(s0.elevation_thr) == list(s1.elevation_thr)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    for i in range(12):
        assert np.array_equal(first[i][0], np.sort(h.ground_indices(i)))
        assert np.array_equal(first[i][1], h.normals(i), equal_nan=True)


def test_full_size_batch_properties(kitti, oracle, golden):
    """BASELINE.json configs[2] at its full size (1024 replayed frames, device-resident, one-pass
    binning, the 64 / 2 patches-per-wave plan, the default schedule of frame ranges over three streams): every replay
    of a source frame gives the same counts and planes as its first occurrence, every frame is partitioned, nothing was
    redone -- and the frames of the batch ARE the oracle's: the first six and a sample from both frame ranges are
    compared with the CPU restatement bit for bit and with the reference build's ground masks (IoU == 1.0)."""
    import torch
    F = 1024
    dev = torch.device("cuda", 0)
    src = [torch.from_numpy(k).to(dev) for k in kitti]
    ptrs = [src[i % 6].data_ptr() for i in range(F)]
    ns = [kitti[i % 6].shape[0] for i in range(F)]
    h = pwpp_hip.Handle()
    b = h.make_device_batch(ptrs, ns)
    h.launch_device_batch(b, cols=4, mode=pwpp_hip.MODE_FRESH)
    h.synchronize()
    counts = h.all_counts()
    for i in range(F):
        assert tuple(counts[i, :3]) == tuple(counts[i % 6, :3])
        assert counts[i, 0] + counts[i, 1] + counts[i, 5] == ns[i]
    for i in (6, 511, 1023):
        assert np.array_equal(np.sort(h.ground_indices(i)), np.sort(h.ground_indices(i % 6)))
        assert np.array_equal(h.normals(i), h.normals(i % 6), equal_nan=True)
    assert h.one_pass_stats() == (1, 0)
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(k) for k in kitti]
    for i in (0, 1, 2, 3, 4, 5, 257, 510, 515, 770, 1022):
        assert_frame_equal(h, i, refs[i % 6], ns[i])
        mask = np.packbits(ground_mask(h.ground_indices(i), ns[i]))
        assert np.array_equal(mask, golden["f32/fresh/%d/ground_mask" % (i % 6)])
    single = pwpp_hip.Handle()
    single.estimate_ground_batch([kitti[3]], mode=pwpp_hip.MODE_FRESH)
    assert np.array_equal(np.sort(single.ground_indices(0)), np.sort(h.ground_indices(3)))  # latency plan, two-pass binning


def test_reference_output_order(kitti, oracle):
    """with PWPP_ORDER_REFERENCE the index lists come out in the reference's order --
    parts in bin traversal order (always), and inside a patch's part the order of the z-sorted bin:
    ascending z, the points removed by R-VPF first in the non-ground part.  The oracle emits the
    reference's own order; the only freedom is among points of equal z, where the reference's
    unstable std::sort leaves the order to libstdc++ and the contract says cloud order: the lists
    equal the oracle's with that one freedom settled (list_order_ref.expected_lists), entry for entry."""
    import list_order_ref
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(7, beams=48, azimuth_steps=1500), 7)
    frames = [kitti[0], kitti[3], syn, kitti[5], kitti[1], kitti[2]]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p) for p in frames]
    h = pwpp_hip.Handle()
    h.set_output_order(True)
    dense = pwpp_synth.make_dense_cloud(77)   # bins of 10-30 k points: parts far beyond one 4096-entry tile (merge passes)
    refs.append(ol.Estimator(oracle, arith=ol.ARITH_FXP).run(dense))
    want = [list_order_ref.expected_lists(p, r) for p, r in zip(frames + [dense], refs)]
    for batch in ([frames[0]], frames, [dense]):   # latency plan + two-pass binning, a batch (one-pass binning), long lists
        h.estimate_ground_batch(batch, mode=pwpp_hip.MODE_FRESH)
        for i, pts in enumerate(batch):
            ground, nonground = want[6] if batch[0] is dense else want[i]
            assert np.array_equal(h.ground_indices(i), ground), "the ground list is not the reference's with ties in cloud order"
            assert np.array_equal(h.nonground_indices(i), nonground), "the non-ground list is not the reference's with ties in cloud order"
            # getGround()/getNonground() rows stay aligned with the index lists
            assert np.array_equal(h.ground(i), pts[h.ground_indices(i), :3])
    h.set_output_order(False)
    h.estimate_ground_batch([frames[0]], mode=pwpp_hip.MODE_FRESH)
    assert np.array_equal(np.sort(h.ground_indices(0)), np.sort(refs[0].ground_idx))


@pytest.mark.parametrize("flags", ["16384", "32768"])
def test_lowest_point_selection_fallbacks(kitti, oracle, flags):
    """The one-pass selection of the num_lpr lowest points falls back to a gather pass (a lane held
    more than four of them) and, if that overflows, to an exact extraction by distinct values (streamed
    rows) or a radix select (four-waves-per-patch kernel).  The fall-backs are rare on real clouds, so
    the debug_flags option (16384 / 32768) forces them for every patch: the results must not change."""
    frames = [kitti[0], kitti[4], kitti[2], kitti[1], kitti[5], kitti[3]]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p) for p in frames]
    h = pwpp_hip.Handle()
    h.set_option("debug_flags", flags)
    for plan in ("W16:1023,W64.2:65535", "S16:255,S64:65535", "B64:65535", "H64:511"):
        h.set_option("fit_plan", plan)
        h.estimate_ground_batch(frames[:5] if plan[0] in "BH" else frames, mode=pwpp_hip.MODE_FRESH)
        for i in range(5):
            assert_frame_equal(h, i, refs[i], frames[i].shape[0])


def test_size_extremes(oracle):
    """The largest frame the C-ABI accepts (4 194 304 points: bins far beyond 65 535 points go to the
    workgroup kernel with its 128-bit lane sums) and a batch of 60 tiny frames around one of 2 M points (the one-pass capacities
    follow the largest frame); bit-exact against the oracle."""
    rng = np.random.default_rng(3)
    base = pwpp_synth.make_cloud(5, beams=64, azimuth_steps=2000)
    reps = 4194304 // base.shape[0] + 1
    big = np.concatenate([base + rng.normal(0, 0.01, base.shape).astype(np.float32) for _ in range(reps)])[:4194304]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch([big], mode=pwpp_hip.MODE_FRESH)
    big_ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(big)
    assert_frame_equal(h, 0, big_ref, big.shape[0])
    for plan in ("H64:1023", "B64:65535"):  # the four-waves-per-patch body on bins of ~10^5 points
        h.set_option("fit_plan", plan)
        h.estimate_ground_batch([big], mode=pwpp_hip.MODE_FRESH)
        assert_frame_equal(h, 0, big_ref, big.shape[0])
    tiny = [base[rng.choice(base.shape[0], 800, replace=False)] for _ in range(60)]
    mix = tiny[:30] + [big[:2000000]] + tiny[30:]
    h2 = pwpp_hip.Handle()
    h2.estimate_ground_batch(mix, mode=pwpp_hip.MODE_FRESH)
    counts = h2.all_counts()
    for i, pts in enumerate(mix):
        assert counts[i, 0] + counts[i, 1] + counts[i, 5] == pts.shape[0]
    for i in (5, 30, 60):
        assert_frame_equal(h2, i, ol.Estimator(oracle, arith=ol.ARITH_FXP).run(mix[i]), mix[i].shape[0])


@pytest.mark.parametrize("flags", [0, 128])
def test_long_sequence_history_trimming(kitti, oracle, flags):
    """60 consecutive frames on one stateful object and on six lock-step streams: the A-GLE histories
    outgrow max_elevation_storage / max_flatness_storage (1000) after ~25 frames, so the front of the
    history is erased every frame from then on (ref :354-355, :372-373); thresholds, sensor height and
    the histories themselves must keep following the sequential oracle bit for bit.  flags = 128: the first
    pass of the history statistics as the reference's sequential sum; 0: its exact shortcut (k_gle_tgr: the
    entries are float values a few binades apart, so no order of summation rounds) -- both are the oracle's."""
    h = pwpp_hip.Handle()
    h.set_option("debug_flags", flags)
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for t in range(60):
        pts = kitti[t % 6]
        h.estimate_ground(pts)
        ref = est.run(pts)
        if t % 7 == 0 or t > 54:
            assert_frame_equal(h, 0, ref, pts.shape[0], state_index=0)
        else:
            st = h.state(0)
            assert st.sensor_height == ref.sensor_height and list(st.elevation_thr) == list(ref.elevation_thr)
            assert list(st.flatness_thr) == list(ref.flatness_thr)
    assert max(len(a) for a in ref.hist_elev) == 1000   # the trimming really happened
    S = 6
    hs = pwpp_hip.Handle()
    hs.set_option("debug_flags", flags)
    hs.set_num_streams(S)
    ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(S)]
    for t in range(45):
        frames = [kitti[(s + t) % 6] for s in range(S)]
        hs.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
        refs = [ests[s].run(frames[s]) for s in range(S)]
        if t % 11 == 0 or t > 41:
            for s in range(S):
                assert_frame_equal(hs, s, refs[s], frames[s].shape[0], state_index=s)


def test_history_statistics_shortcut_only_where_it_is_exact(kitti):
    """k_gle_tgr sums a history in parallel where that cannot round (float-valued entries a few binades apart) and as the
    reference's sequential sum everywhere else.  Histories restored from a checkpoint may hold anything: here a sum that
    cancels (1e16 + 1 - 1e16 + 1 ... depends on its order), entries that are no floats (0.1) and a flatness history that
    spans 40 binades.  The kernel must notice and sum them in order: the state after the next frame equals that of a handle
    whose shortcut is switched off (debug flag 128)."""
    elev = np.array([1e16, 1.0, -1e16, 1.0] * 200 + [0.1] * 100)
    flat = np.array([1e-12, 3.0, 0.1, 2.5e-7] * 225)
    seen = []
    for flags in (0, 128):
        h = pwpp_hip.Handle()
        h.set_option("debug_flags", flags)
        h.set_num_streams(1)
        h.estimate_ground_batch([kitti[0]], mode=pwpp_hip.MODE_STREAMS)
        for ring in range(4):
            h.set_history(0, 0, ring, elev[ring:])
            h.set_history(0, 1, ring, flat[:len(flat) - 3 * ring])
        for t in (1, 2):
            h.estimate_ground_batch([kitti[t]], mode=pwpp_hip.MODE_STREAMS)
        st = h.state(0)
        seen.append((st.sensor_height, list(st.elevation_thr), list(st.flatness_thr),
                     [h.history(0, w, r).tobytes() for w in range(2) for r in range(4)], np.sort(h.ground_indices(0)).tobytes()))
    assert seen[0] == seen[1]


def test_k5_in_two_launches_leaves_the_same_state(kitti, oracle):
    """Up to 64 stateful streams run K5 in two launches (option split_k5, default 1): the index lists wait for the first part only, the
    statistics over the A-GLE histories run on the handle's second stream and are joined before the next call and before the host reads
    anything.  Three streams, ten steps from restored histories long enough to be trimmed every frame: thresholds, sensor height, histories
    and lists after every step must equal those of a handle whose K5 is one kernel, and the last step the oracle's."""
    rng = np.random.default_rng(5)
    hist = [[(rng.normal(-1.73, 0.05, 990 + 3 * r)).astype(np.float32).astype(np.float64) if w == 0 else
             np.abs(rng.normal(2e-3, 1e-3, 985 + 5 * r)).astype(np.float32).astype(np.float64) for r in range(4)] for w in range(2)]
    S, seen = 3, []
    for split in (1, 0, 2):  # (2: the second launch behind the lists instead of beside K6)
        h = pwpp_hip.Handle()
        h.set_option("split_k5", split)
        h.set_num_streams(S)
        h.estimate_ground_batch([kitti[s] for s in range(S)], mode=pwpp_hip.MODE_STREAMS)
        for s in range(S):
            for w in range(2):
                for r in range(4):
                    h.set_history(s, w, r, hist[w][r][s:])
        trace = []
        for t in range(1, 11):
            h.estimate_ground_batch([kitti[(s + t) % 6] for s in range(S)], mode=pwpp_hip.MODE_STREAMS)
            for s in range(S):
                st = h.state(s)
                trace.append((st.sensor_height, list(st.elevation_thr), list(st.flatness_thr),
                              [h.history(s, w, r).tobytes() for w in range(2) for r in range(4)],
                              np.sort(h.ground_indices(s)).tobytes(), np.sort(h.nonground_indices(s)).tobytes()))  # (the lists' order is the scatter's)
        seen.append(trace)
        h.close()
    assert seen[0] == seen[1] and seen[0] == seen[2]
    # ... and a stream that starts from nothing follows the oracle through the split kernel (its first frames take their statistics from
    # the histories read back, not from the LDS copy of a frame that starts from empty histories)
    h = pwpp_hip.Handle()
    h.set_num_streams(1)
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for t in range(4):
        h.estimate_ground_batch([kitti[t]], mode=pwpp_hip.MODE_STREAMS)
        ref = est.run(kitti[t])
        assert_frame_equal(h, 0, ref, kitti[t].shape[0], state_index=0)


def test_history_statistics_of_a_big_stream_batch_equal_the_single_stream_kernel(kitti):
    """k_gle_tgr has two variants: up to 64 frames a workgroup stages a whole 1000-entry history in one LDS tile (the variant the
    long-sequence tests hold against the oracle), larger batches walk it in tiles of 496 entries, fetched two entries per load
    while the tile before is summed.  Here stream 0 of a 70-stream batch and a single stream start from the same restored
    histories (900-1030 float-valued entries: two to three tiles, trimming included) and see the same two frames: thresholds,
    sensor height, histories and ground sets must be identical."""
    rng = np.random.default_rng(77)
    hist = [[(rng.normal(-1.73, 0.05, 900 + 37 * r + 11 * w)).astype(np.float32).astype(np.float64) if w == 0 else
             np.abs(rng.normal(2e-3, 1e-3, 905 + 29 * r)).astype(np.float32).astype(np.float64) for r in range(4)] for w in range(2)]
    got = []
    for S in (70, 1):
        h = pwpp_hip.Handle()
        h.set_num_streams(S)
        h.estimate_ground_batch([kitti[(s + 3) % 6] for s in range(S)], mode=pwpp_hip.MODE_STREAMS)  # (the streams exist now)
        for w in range(2):
            for r in range(4):
                h.set_history(0, w, r, hist[w][r])
        for t in (1, 2):
            h.estimate_ground_batch([kitti[t]] + [kitti[(s + t) % 6] for s in range(1, S)], mode=pwpp_hip.MODE_STREAMS)
        st = h.state(0)
        got.append((st.sensor_height, list(st.elevation_thr), list(st.flatness_thr),
                    [h.history(0, w, r).tobytes() for w in range(2) for r in range(4)], np.sort(h.ground_indices(0)).tobytes()))
    assert got[0] == got[1]
    assert max(len(x) for x in got[0][3]) // 8 == 1000  # (the longest histories were trimmed to max_*_storage on the way)


def test_handle_reuse_across_modes_and_sizes(kitti, oracle):
    """One handle, interleaved: lock-step streams, a fresh batch (one-pass), a single fresh frame, a
    bigger fresh batch, reference-order mode on and off.  The streams' adaptive state lives in its own
    slabs and must not notice any of it; every result equals the oracle's."""
    S = 3
    h = pwpp_hip.Handle()
    h.set_num_streams(S)
    ests = [ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(S)]
    fresh_refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(k) for k in kitti]

    def step(t):
        frames = [kitti[(s + t) % 6] for s in range(S)]
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
        for s in range(S):
            assert_frame_equal(h, s, ests[s].run(frames[s]), frames[s].shape[0], state_index=s)

    step(0)
    step(1)
    h.estimate_ground_batch([kitti[i % 6] for i in range(7)], mode=pwpp_hip.MODE_FRESH)
    for i in range(7):
        assert_frame_equal(h, i, fresh_refs[i % 6], kitti[i % 6].shape[0], check_state=False)
    step(2)
    h.set_output_order(True)
    h.estimate_ground_batch([kitti[4]], mode=pwpp_hip.MODE_FRESH)
    assert np.array_equal(kitti[4][h.ground_indices(0), 2], kitti[4][np.asarray(fresh_refs[4].ground_idx), 2])
    step(3)
    h.set_output_order(False)
    h.estimate_ground_batch([kitti[i % 6] for i in range(20)], mode=pwpp_hip.MODE_FRESH)
    assert_frame_equal(h, 19, fresh_refs[1], kitti[1].shape[0], check_state=False)
    step(4)


def test_handles_on_concurrent_host_threads(kitti, oracle):
    """SURVEY section 8b, threading: distinct objects are independent (the reference has no globals), so
    four host threads each drive their own handle -- a stateful sequence, then a fresh batch big enough
    for the one-pass binning -- at the same time (ctypes drops the GIL around every call).  Results are
    collected inside the threads and compared with the oracle afterwards."""
    import threading
    T = 4
    seq_refs, fresh_refs = [], [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(k) for k in kitti]
    for t in range(T):
        est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
        seq_refs.append([est.run(kitti[(t + j) % 6]) for j in range(4)])
    got, errors = [None] * T, []

    def worker(t):
        try:
            h = pwpp_hip.Handle()
            out = []
            for j in range(4):
                h.estimate_ground(kitti[(t + j) % 6])
                out.append((np.sort(h.ground_indices(0)), h.normals(0).copy(), h.height()))
            order = [(t + i) % 6 for i in range(6 + t)]
            h.estimate_ground_batch([kitti[k] for k in order], mode=pwpp_hip.MODE_FRESH)
            batch = [(np.sort(h.ground_indices(i)), h.normals(i).copy()) for i in range(len(order))]
            got[t] = (out, order, batch)
        except Exception as e:  # surfaced on the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(T):
        out, order, batch = got[t]
        for j, (gi, nrm, height) in enumerate(out):
            ref = seq_refs[t][j]
            assert np.array_equal(gi, np.sort(np.asarray(ref.ground_idx))) and height == ref.sensor_height
            assert np.array_equal(nrm, ref.normals, equal_nan=True)
        for (gi, nrm), k in zip(batch, order):
            assert np.array_equal(gi, np.sort(np.asarray(fresh_refs[k].ground_idx)))
            assert np.array_equal(nrm, fresh_refs[k].normals, equal_nan=True)


def test_overlap_mode_two_frame_ranges_on_two_streams(kitti, oracle):
    """pwpp_set_overlap: a batch of 128+ frames runs as two frame ranges with their own launches on the handle's
    two streams (shared workspaces, shifted base pointers).  Fresh batch (one-pass binning, odd frame count)
    and lock-step streams over several steps: every sampled frame bit-exact against the oracle, every frame
    partitioned, replays agree."""
    F = 301
    frames = [kitti[i % 6] for i in range(F)]
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(k) for k in kitti]
    h = pwpp_hip.Handle()
    h.set_overlap(True)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    counts = h.all_counts()
    for i in range(F):
        assert tuple(counts[i, :3]) == tuple(counts[i % 6, :3])
        assert counts[i, 0] + counts[i, 1] + counts[i, 5] == frames[i].shape[0]
    for i in (0, 5, 150, 151, 152, 159, 160, 161, 299, 300):   # both sides of the split (152 = 19 groups of eight)
        assert_frame_equal(h, i, refs[i % 6], frames[i].shape[0], check_state=False)
    assert h.one_pass_stats()[1] == 0
    # a wedge-shaped cloud in the second range overflows its bin segments: the whole batch is redone on the two-pass
    # path, again as two ranges
    rng = np.random.default_rng(5)
    wedge = kitti[0].copy()
    sel = rng.random(wedge.shape[0]) < 0.7
    r = np.hypot(wedge[sel, 0], wedge[sel, 1])
    a = rng.uniform(0.1, 0.27, sel.sum())
    wedge[sel, 0] = (r * np.cos(a)).astype(np.float32)
    wedge[sel, 1] = (r * np.sin(a)).astype(np.float32)
    odd = frames[:200] + [wedge] + frames[:39]
    h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
    assert h.one_pass_stats() == (2, 1)
    assert h.redo_stats() == (F + 240, 1)  # (round 5: the wedge alone is redone, in place)
    assert_frame_equal(h, 200, ol.Estimator(oracle, arith=ol.ARITH_FXP).run(wedge), wedge.shape[0], check_state=False)
    for i in (0, 119, 120, 199, 201, 239):
        assert_frame_equal(h, i, refs[(i if i < 200 else i - 201) % 6], odd[i].shape[0], check_state=False)
    S = 130
    hs = pwpp_hip.Handle()
    hs.set_num_streams(S)
    hs.set_overlap(True)
    sample = (0, 63, 64, 71, 72, 129)
    ests = {s: ol.Estimator(oracle, arith=ol.ARITH_FXP) for s in sample}
    for t in range(3):
        fr = [kitti[(s + t) % 6] for s in range(S)]
        hs.estimate_ground_batch(fr, mode=pwpp_hip.MODE_STREAMS)
        for s in sample:
            assert_frame_equal(hs, s, ests[s].run(fr[s]), fr[s].shape[0], state_index=s)


def test_error_reporting_on_the_device(kitti):
    """Misuse comes back as an error code + message (RuntimeError in Python), never as a wrong result:
    more frames than streams, a misaligned device buffer, unsupported parameters, reading results
    before anything ran -- and the handle keeps working afterwards."""
    import torch
    h = pwpp_hip.Handle()
    with pytest.raises(pwpp_hip.PwppError, match="no frame"):
        h.ground_indices(0)
    with pytest.raises(pwpp_hip.PwppError, match="streams"):
        h.estimate_ground_batch([kitti[0], kitti[1]], mode=pwpp_hip.MODE_STREAMS)   # one stream by default
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(kitti[0]).to(dev)
    with pytest.raises(pwpp_hip.PwppError, match="aligned"):
        h.estimate_ground_batch_device([t.data_ptr() + 4], [100])
    with pytest.raises(pwpp_hip.PwppError, match="order"):
        h._check(h._L.pwpp_set_output_order(h._h, 7))
    for bad in (dict(num_zones=3), dict(num_iter=0), dict(num_lpr=257), dict(max_range=1.0, min_range=2.0), dict(max_range=1e7)):
        p = pwpp_hip.default_params()
        for k, v in bad.items():
            setattr(p, k, v)
        with pytest.raises(pwpp_hip.PwppError):
            pwpp_hip.Handle(p)
    with pytest.raises(pwpp_hip.PwppError, match="share one probe array"):   # (the two sets of timing probes)
        h.set_option("debug_flags", 4 | 8)
    for removed in ("fuse_scan", "cu_split", "fit_concurrent", "overlap_mode", "bin_block"):
        with pytest.raises(pwpp_hip.PwppError, match="unknown option"):
            h.set_option(removed, "1")
    h.estimate_ground(kitti[0])   # still usable
    assert h.counts(0)[0] + h.counts(0)[1] == kitti[0].shape[0]
    with pytest.raises(pwpp_hip.PwppError, match="out of range"):
        h.ground_indices(3)


def test_schedules_give_one_result(kitti, oracle):
    """The same 136-frame batch through every schedule the library has -- one stream, the in-handle overlap schedule, four frame
    ranges -- and two handles with a batch each in flight: identical counts everywhere, spot frames identical to the oracle; and
    single frames of a default handle identical to the oracle."""
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(k) for k in kitti]
    F = 136
    frames = [kitti[i % 6] for i in range(F)]
    h = pwpp_hip.Handle()
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    want = h.all_counts().copy()
    for i in (0, 67, 135):
        assert_frame_equal(h, i, refs[i % 6], frames[i].shape[0], check_state=False)
    for setup in (lambda: h.set_overlap(False), lambda: h.set_overlap(True), lambda: h.set_option("overlap_ranges", 4)):
        setup()
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        assert np.array_equal(h.all_counts(), want)
        assert_frame_equal(h, 101, refs[101 % 6], frames[101].shape[0], check_state=False)
    h2 = pwpp_hip.Handle()
    for hh in (h, h2):
        hh.set_overlap(False)
    import torch
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(f).to(dev) for f in kitti]
    ptrs, ns = [bufs[i % 6].data_ptr() for i in range(F)], [kitti[i % 6].shape[0] for i in range(F)]
    b1, b2 = h.make_device_batch(ptrs, ns), h2.make_device_batch(ptrs, ns)
    for k in range(6):  # two batches in flight, as bench.py's timed region
        hh, bb = (h, b1) if k % 2 == 0 else (h2, b2)
        if k >= 2:
            hh.synchronize()
        hh.launch_device_batch(bb, cols=4, mode=pwpp_hip.MODE_FRESH)
    for hh in (h, h2):
        hh.synchronize()
        assert np.array_equal(hh.all_counts(), want)
        assert_frame_equal(hh, 29, refs[29 % 6], frames[29].shape[0], check_state=False)
    # ... and the library's own pipe (pwpp_pipe_*): two batches in flight, two different batches alternating; the handle a submit
    # returns holds that batch's results until it comes round again
    frames_b = [kitti[(i + 3) % 6] for i in range(F)]
    bufs_b = [bufs[(i + 3) % 6] for i in range(F)]
    pipe = pwpp_hip.Pipe(depth=2)
    ba = pipe.handle(0).make_device_batch(ptrs, ns)
    bb = pipe.handle(0).make_device_batch([t.data_ptr() for t in bufs_b], [f.shape[0] for f in frames_b])
    holders = [pipe.submit_device_batch(ba if k % 2 == 0 else bb) for k in range(5)]
    assert holders[0]._h.value == holders[2]._h.value == holders[4]._h.value != holders[1]._h.value == holders[3]._h.value
    pipe.drain()
    assert np.array_equal(holders[4].all_counts(), want)                      # batch a
    assert_frame_equal(holders[4], 77, refs[77 % 6], frames[77].shape[0], check_state=False)
    assert_frame_equal(holders[3], 77, refs[(77 + 3) % 6], frames_b[77].shape[0], check_state=False)  # batch b
    with pytest.raises(pwpp_hip.PwppError, match="depth"):
        pwpp_hip.Pipe(depth=9)
    view = holders[4]
    pipe.close()
    with pytest.raises(pwpp_hip.PwppError):  #  a view of a closed pipe's handle fails, it does not touch the freed handle
        view.counts(0)
    one = pwpp_hip.Handle()
    for k in (1, 2, 4, 5):
        one.estimate_ground_batch([kitti[k]], mode=pwpp_hip.MODE_FRESH)
        assert_frame_equal(one, 0, refs[k], kitti[k].shape[0])


def test_cpp_class_with_eigen_types(kitti, golden, tmp_path):
    """The reference's exact C++ signatures (Eigen::MatrixXf in, Eigen::MatrixX3f / Eigen::VectorXi out)
    of the class mirror.  Eigen is not in this image; the program is compiled against the test
    infrastructure's stand-in for the Eigen API (oracle/eigen_shim, column-major like Eigen)."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "patchwork-plusplus_amd")
    exe = str(tmp_path / "demo_eigen")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(root, "oracle", "eigen_shim"), "-I", os.path.join(pkg, "include"),
                    "-I", os.path.join(root, "include"), "-o", exe, os.path.join(pkg, "examples", "demo_eigen.cpp"),
                    "-L", os.path.join(pkg, "lib"), "-lpwpp_hip", "-Wl,-rpath," + os.path.join(pkg, "lib")], check=True)
    path = tmp_path / "000000.bin"
    kitti[0].tofile(path)
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout
    ng = int(re.search(r"Ground Points\s+#: (\d+)", out).group(1))
    nn = int(re.search(r"Nonground Points #: (\d+)", out).group(1))
    npatch = int(re.search(r"patches: (\d+)", out).group(1))
    assert [ng, nn, npatch] == list(golden["f32/fresh/0/counts"])
    assert "aligned: 1" in out
    assert "nz0 == normals(0,2), x0 == ground(0,0), transpose 3x%d" % ng in out
    assert re.search(r"Time taken : [0-9.e+-]+\(sec\) ~ [0-9.e+-]+\(czm\) \+ 0\(sort\) \+ [0-9.e+-]+\(pca\) \+ [0-9.e+-]+\(estimate\)", out)
    assert "Estimation is finished" in out


def test_histories_that_the_reference_never_trims(oracle):
    """A sensor that sees no ground in ring 0: update_flatness_thr stops at ring 0 ("break", ref :363-364), so the
    flatness histories of rings 1-3 are never trimmed and grow by up to 32 + 54 + 54 entries a frame -- unbounded
    vectors in the reference.  The history slabs (max storage + 1024 at first) must grow with them: 150 frames on one
    stream, compared with the oracle frame by frame, histories included."""
    base = pwpp_synth.make_cloud(21, beams=48, azimuth_steps=1200)
    r = np.hypot(base[:, 0], base[:, 1])
    far = base[r > 7.7]  # nothing in ring 0 (2.7 .. 7.53 m)
    rng = np.random.default_rng(5)
    h = pwpp_hip.Handle()
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for t in range(150):
        pts = far.copy()
        pts[:, 2] += rng.normal(0, 0.004, len(pts)).astype(np.float32)
        h.estimate_ground(pts)
        ref = est.run(pts)
        if t % 10 == 9 or t > 120:
            assert_frame_equal(h, 0, ref, pts.shape[0], state_index=0)
    assert len(ref.hist_flat[0]) <= 1 and max(len(ref.hist_flat[k]) for k in (1, 2, 3)) > 2100  # beyond the first slab
    assert len(ref.hist_elev[1]) == 1000  # ... while the elevation histories are trimmed every frame


def test_checkpoint_and_restore_a_stream(kitti, oracle):
    """pwpp_get_state / pwpp_get_history -> pwpp_set_state / pwpp_set_history: a stream restored on another handle
    continues bit for bit (set_state used to drop the histories)."""
    a = pwpp_hip.Handle()
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for k in (0, 1, 2, 3):
        a.estimate_ground(kitti[k])
        est.run(kitti[k])
    ck = a.checkpoint(0)
    b = pwpp_hip.Handle()
    b.restore(ck, 0)
    for k in (4, 5, 0):
        b.estimate_ground(kitti[k])
        assert_frame_equal(b, 0, est.run(kitti[k]), kitti[k].shape[0], state_index=0)
    # what a restore refuses: histories the reference could never hold -- non-finite entries; and a PointCloud2
    # blob that does not start on a float boundary
    before = b.history(0, 0, 0)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(pwpp_hip.PwppError):
            b.set_history(0, 0, 0, [0.5, bad, 0.25])
    assert np.array_equal(b.history(0, 0, 0), before)  # (a refused call changes nothing)
    blob = np.zeros(16 * 64 + 8, np.uint8)
    off = (-blob.ctypes.data) % 4 + 1  # one byte past a 4-byte boundary
    with pytest.raises(pwpp_hip.PwppError):
        b.estimate_ground_fields(blob[off:off + 16 * 64], 64, 16, 0, 4, 8)


def test_trim_workspace_and_options(kitti, oracle):
    """pwpp_trim_workspace gives the per-batch buffers back and the next call allocates again; pwpp_set_option rejects
    what it does not know; more than 65535 frames per call are refused up front."""
    h = pwpp_hip.Handle()
    frames = [kitti[k % 6] for k in range(8)]
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    ref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(kitti[1])
    assert_frame_equal(h, 1, ref, kitti[1].shape[0])
    before = h.workspace_bytes()
    h.trim_workspace()
    # (every frames-proportional buffer goes -- what is left is the stream state and the per-handle tables)
    assert before > 8 * kitti[0].shape[0] * 16 and h.workspace_bytes() < 2 << 20
    with pytest.raises(pwpp_hip.PwppError):
        h.ground_indices(0)  # the lists lived in the workspace
    assert h.state(0).sensor_height == pwpp_hip.default_params().sensor_height  # the (untouched) stream state is still readable
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert_frame_equal(h, 1, ref, kitti[1].shape[0])
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("no_such_option", 1)
    with pytest.raises(pwpp_hip.PwppError):
        h.set_option("fit_plan", "rm -rf")
    with pytest.raises(pwpp_hip.PwppError):
        h.estimate_ground_batch([kitti[0][:16]] * 65536, mode=pwpp_hip.MODE_FRESH)


# the parameter set of the reference's ROS 2 launch file (ros/launch/patchworkpp.launch.py:50-64) as the node
# applies it (ros/src/GroundSegmentationServer.cpp:27-46: RNR off, N x 3 input)
ROS_LAUNCH = dict(sensor_height=1.88, num_iter=3, num_lpr=20, num_min_pts=0, th_seeds=0.3, th_dist=0.125, th_seeds_v=0.25,
                  th_dist_v=0.9, max_range=80.0, min_range=1.0, uprightness_thr=0.101, enable_RNR=0)


def pointcloud2_blob(pts, point_step, off, extra_seed=0):
    """A sensor_msgs/PointCloud2 data blob: float32 x, y, z (and intensity) at byte offsets `off` of records of
    point_step bytes, the rest of a record filled with other fields' bytes (ring, time, padding)."""
    rng = np.random.default_rng(extra_seed)
    blob = rng.integers(0, 256, (pts.shape[0], point_step), dtype=np.uint8)
    for k, o in enumerate(off):
        if o >= 0:
            blob[:, o:o + 4] = pts[:, k].astype(np.float32).view(np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(blob)


def test_ros_wrapper_parameters_and_pointcloud2_input(kitti, oracle):
    """SURVEY 8f-f4, the part that can be tested without ROS: (i) the launch file's parameter set as ONE variant,
    on a stateful three-frame sequence of N x 3 clouds (num_min_pts = 0 lets empty bins through: the sequential
    GLE kernel); (ii) the same frames handed over as PointCloud2 blobs (x, y, z at odd offsets of 32-byte and
    18 * 4-byte records, with and without an intensity field), read in place by the binning kernels."""
    p = apply_variant(pwpp_hip.default_params(), ROS_LAUNCH)
    op = to_oracle_params(p)
    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(31, beams=32, azimuth_steps=1200), 31)
    seq = [kitti[2], syn, kitti[3]]
    est = ol.Estimator(oracle, op, arith=ol.ARITH_FXP)
    refs = [est.run(np.ascontiguousarray(c[:, :3])) for c in seq]
    # (i) N x 3 matrices, as PointCloud2ToEigenMat produces them -- and against the REFERENCE BUILD itself (one object of each of
    # its flavours over the sequence): identical ground sets in every frame on which the reference's float and exact-f64
    # builds agree (contract v3: the bins of 0-3 points num_min_pts = 0 lets through follow the reference's float sums)
    h = pwpp_hip.Handle(p)
    rlib, xlib = ol.reference(ol.ARITH_EIGEN_F32), ol.reference(ol.ARITH_EXACT_F64)
    r_est = ol.Estimator(rlib, op, arith=ol.ARITH_EIGEN_F32) if rlib else None
    x_est = ol.Estimator(xlib, op, arith=ol.ARITH_EXACT_F64) if xlib else None
    for c, ref in zip(seq, refs):
        c3 = np.ascontiguousarray(c[:, :3])
        h.estimate_ground(c3)
        assert_frame_equal(h, 0, ref, c.shape[0], state_index=0)
        if r_est and x_est:
            a, b = r_est.run(c3), x_est.run(c3)
            if len(np.setxor1d(a.ground_idx, b.ground_idx)) == 0:
                assert np.array_equal(np.sort(h.ground_indices(0)), np.sort(a.ground_idx)), "ground set differs from the reference build"
    # (ii) the message's data blob, fields in place
    for step, off in ((32, (0, 4, 8, -1)), (32, (4, 12, 20, -1)), (72, (60, 8, 32, -1)), (16, (0, 4, 8, 12))):
        h2 = pwpp_hip.Handle(p)
        for c, ref in zip(seq, refs):
            h2.estimate_ground_fields(pointcloud2_blob(c, step, off, step), c.shape[0], step, *off)
            assert_frame_equal(h2, 0, ref, c.shape[0], state_index=0)
            g = h2.ground_indices(0)
            assert np.array_equal(h2.ground(0), c[g, :3])  # the xyz getters read the same fields
    # with RNR enabled an intensity field is used exactly like the fourth matrix column
    p4 = pwpp_hip.default_params()
    ref4 = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(kitti[1])
    h4 = pwpp_hip.Handle(p4)
    h4.estimate_ground_fields(pointcloud2_blob(kitti[1], 24, (8, 0, 16, 4), 1), kitti[1].shape[0], 24, 8, 0, 16, 4)
    assert_frame_equal(h4, 0, ref4, kitti[1].shape[0], state_index=0)
    for bad in ((10, 0, 4, 8, -1), (16, 0, 4, 14, -1), (16, 0, 4, 8, 13), (8, 0, 4, 8, -1)):
        with pytest.raises(pwpp_hip.PwppError):
            h4.estimate_ground_fields(np.zeros(64, np.uint8), 1, *bad)


def test_ros_node_core(kitti, oracle, tmp_path):
    """the ROS 2 node's logic -- patchwork-plusplus_amd/ros/include/patchworkpp_ros/segmentation_core.hpp, everything
    between "a PointCloud2 arrived" and "three PointCloud2 payloads are ready" -- built and run WITHOUT ROS
    (examples/ros_core_demo.cpp): three KITTI frames as 32-byte-per-point message payloads with x, y, z between other fields,
    one long-lived node core with the launch file's parameter set.  The payloads it would publish (cloud, ground, non-ground:
    x, y, z float32 + 4 bytes, the reference's CreatePointCloud2Msg layout) are compared -- the cloud byte for byte, the two
    lists as multisets of points, through checksums -- with what the oracle (stateful, same parameters, N x 3 input as PointCloud2ToEigenMat gives) implies.
    The rclcpp component around the core (ros/src/ground_segmentation_server.cpp) needs ROS 2 and is not built here."""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "patchwork-plusplus_amd", "examples", "ros_core_demo")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "patchwork-plusplus_amd"), "examples/ros_core_demo"], check=True)
    paths = []
    for k in range(3):
        p = tmp_path / ("%06d.bin" % k)
        kitti[k].tofile(p)
        paths.append(str(p))
    out = subprocess.run([exe] + paths, capture_output=True, text=True, check=True).stdout
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 3, out

    def fnv1a(b):
        h = 1469598103934665603
        for x in b:
            h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % h

    def point_sum(b):  # the lists as multisets of 16-byte points (their order inside a patch is the scatter order: not reproducible)
        h = np.full(len(b) // 16, 1469598103934665603, np.uint64)
        a = np.frombuffer(b, np.uint8).reshape(-1, 16).astype(np.uint64)
        with np.errstate(over="ignore"):
            for j in range(16):
                h = (h ^ a[:, j]) * np.uint64(1099511628211)
            return "%016x" % int(h.sum(dtype=np.uint64))

    def payload(xyz):  # CreatePointCloud2Msg: point_step 16
        a = np.zeros((xyz.shape[0], 4), np.float32)
        a[:, :3] = xyz
        return a.tobytes()

    prm = apply_variant(pwpp_hip.default_params(), ROS_LAUNCH)
    h = pwpp_hip.Handle(prm)  # the same sequence through the C-ABI: the lists' ORDER inside a patch is the library's own, so
    est = ol.Estimator(oracle, to_oracle_params(prm), arith=ol.ARITH_FXP)  # the payload bytes are compared with the library, the sets with the oracle
    for k, line in enumerate(lines):
        c3 = np.ascontiguousarray(kitti[k][:, :3])
        h.estimate_ground(c3)
        ref = est.run(c3)
        assert_frame_equal(h, 0, ref, c3.shape[0], state_index=0)
        assert line["points"] == c3.shape[0] and line["cloud"] == [c3.shape[0], 16, fnv1a(payload(c3))]
        g, ng = h.ground(0), h.nonground(0)
        assert line["ground"][:2] == [len(ref.ground_idx), 16] and line["nonground"][:2] == [len(ref.nonground_idx), 16]
        assert line["ground"][2] == point_sum(payload(g)) and line["nonground"][2] == point_sum(payload(ng))
    #  a message whose step / offsets are not multiples of four is repacked, same payloads; a field that reaches
    # beyond point_step is refused (the node logs and drops such a message)
    odd = subprocess.run([exe, "--layout=odd"] + paths, capture_output=True, text=True, check=True).stdout
    odd_lines = [json.loads(l) for l in odd.splitlines() if l.startswith("{")]
    assert [(l["cloud"], l["ground"], l["nonground"]) for l in odd_lines] == [(l["cloud"], l["ground"], l["nonground"]) for l in lines]
    bad = subprocess.run([exe, "--layout=bad"] + paths[:1], capture_output=True, text=True)
    assert bad.returncode == 1 and "outside point_step" in bad.stdout


def test_plane_members_carry_over_between_frames(kitti, oracle):
    """The reference object's plane members (normal_, pc_mean_, singular_values_, d_) survive from call to call, and with
    num_min_pts = 0 (the ROS launch file) a bin without points is "processed" and reports them: for a sensor with a
    blind sector the first bins of frame k carry the plane the LAST bin of frame k - 1 was fitted with.  Sequences of a
    stream, lock-step streams (one of them with the blind sector), a one-pass batch of streams, and a stream
    checkpointed after two frames and continued on another handle -- against the oracle, which keeps the members as
    the reference does."""
    p = apply_variant(pwpp_hip.default_params(), ROS_LAUNCH)
    op = to_oracle_params(p)

    def blind(c, lo_deg, hi_deg):
        a = np.degrees(np.arctan2(c[:, 1], c[:, 0])) % 360.0
        return np.ascontiguousarray(c[~((a >= lo_deg) & (a < hi_deg)), :3])

    seq = [blind(kitti[k], 0.0, 70.0) for k in range(5)]  # sectors 0-2 of zone 0 and more see nothing
    est = ol.Estimator(oracle, op, arith=ol.ARITH_FXP)
    refs = [est.run(c) for c in seq]
    assert any(r.records["n_points"][0] == 0 for r in refs[1:]), "the first processed bin should be an empty one"
    h = pwpp_hip.Handle(p)
    for k, (c, ref) in enumerate(zip(seq, refs)):
        h.estimate_ground(c)
        assert_frame_equal(h, 0, ref, c.shape[0], state_index=0)
        if k == 1:
            ck = h.checkpoint(0)
    assert np.abs(h.plane_state(0)[3:6]).max() > 0  # some plane is in the members
    h2 = pwpp_hip.Handle(p)   # ... continued elsewhere from the checkpoint
    h2.restore(ck, 0)
    for c, ref in zip(seq[2:], refs[2:]):
        h2.estimate_ground(c)
        assert_frame_equal(h2, 0, ref, c.shape[0], state_index=0)
    # lock-step streams, small (two-pass binning) and as a one-pass batch of six streams
    for streams in (2, 6):
        hs = pwpp_hip.Handle(p)
        hs.set_num_streams(streams)
        ests = [ol.Estimator(oracle, op, arith=ol.ARITH_FXP) for _ in range(streams)]
        for step in range(3):
            frames = [blind(kitti[(step + i) % 6], 0.0, 70.0) if i % 2 == 0 else np.ascontiguousarray(kitti[(step + i) % 6][:, :3])
                      for i in range(streams)]
            hs.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
            for i, c in enumerate(frames):
                assert_frame_equal(hs, i, ests[i].run(c), c.shape[0])


def test_patches_that_start_from_the_plane_fitted_before_them(kitti, oracle):
    """A patch whose first fit set is empty consults whatever plane the reference object fitted last (patchworkpp.cpp:49:
    the members survive from patch to patch and frame to frame).  It takes a lowest height of -inf, a lone height so large
    that th_seeds is absorbed (1e30 m in a one-point patch), or num_lpr = 0 -- the parallel fit kernels recognise the
    case, K5 / K6 leave the frame alone and the host finishes it with the serial k_fit_fixup.  Fresh batches under several
    plans, a stateful sequence (the first dirty patch of a frame starts from the last plane of the frame before) and
    lock-step streams, against the oracle."""
    rng = np.random.default_rng(5)

    def spoil(c, k):
        c = c.copy()
        pick = rng.choice(c.shape[0], k, replace=False)
        c[pick, 2] = -np.inf                      # lowest height of its bin, wherever it falls
        lone = np.array([[70.0, 30.0 + i, 1e30, 0.5] for i in range(3)] + [[3.5, -1.0, 3e38, 0.5]], np.float32)
        return np.ascontiguousarray(np.concatenate([c, lone[:, :c.shape[1]]]))

    syn = pwpp_synth.add_edge_cases(pwpp_synth.make_cloud(77, beams=32, azimuth_steps=1200), 77)
    frames = [spoil(kitti[0], 40), spoil(syn, 25), kitti[1], spoil(kitti[5], 3)]
    for variant in (dict(), dict(num_min_pts=1), dict(num_min_pts=0), dict(num_lpr=0), dict(enable_RVPF=0, num_min_pts=1)):
        p = apply_variant(pwpp_hip.default_params(), variant)
        op = to_oracle_params(p)
        refs = [ol.Estimator(oracle, op, arith=ol.ARITH_FXP).run(c) for c in frames]
        for plan in ("", "W16:1023,W64.2:65535", "S16:255,S64:65535", "B64:65535", "S16:100"):
            h = pwpp_hip.Handle(p)
            if plan:
                h.set_option("fit_plan", plan)
            h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
            for i, c in enumerate(frames):
                assert_frame_equal(h, i, refs[i], c.shape[0])
            assert h.fixed_up_frames() >= 1
        # one stream, frame after frame; then two streams in lock step
        est = ol.Estimator(oracle, op, arith=ol.ARITH_FXP)
        h = pwpp_hip.Handle(p)
        for c in frames + frames[:2]:
            h.estimate_ground(c)
            assert_frame_equal(h, 0, est.run(c), c.shape[0], state_index=0)
        hs = pwpp_hip.Handle(p)
        hs.set_num_streams(2)
        ests = [ol.Estimator(oracle, op, arith=ol.ARITH_FXP) for _ in range(2)]
        for step in range(3):
            pair = [frames[step], frames[(step + 2) % 4]]
            hs.estimate_ground_batch(pair, mode=pwpp_hip.MODE_STREAMS)
            for i, c in enumerate(pair):
                assert_frame_equal(hs, i, ests[i].run(c), c.shape[0])
    clean = pwpp_hip.Handle()
    clean.estimate_ground_batch(kitti, mode=pwpp_hip.MODE_FRESH)
    assert clean.fixed_up_frames() == 0  # real scans never take the path


def test_dense_batch_one_pass_36_sectors(oracle):
    """BASELINE.json configs[4] as a BATCH (bench.py --workload dense): 32 dense 128-beam ~480 k-point frames,
    36-sector CZM, one-pass binning, overlap off and on; every frame against the oracle (only a
    single frame was compared)."""
    p = pwpp_hip.default_params()
    for k in range(4):
        p.num_sectors_each_zone[k] = 36
    src = [pwpp_synth.make_dense_cloud(1000 + k) for k in range(4)]
    refs = [ol.Estimator(oracle, to_oracle_params(p), arith=ol.ARITH_FXP).run(c) for c in src]
    frames = [src[i % 4] for i in range(32)]
    h = pwpp_hip.Handle(p)
    h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
    assert h.one_pass_stats() == (1, 0)
    for i in range(32):
        assert_frame_equal(h, i, refs[i % 4], frames[i].shape[0])
    big = [src[i % 4] for i in range(128)]  # 128 frames: two frame ranges on two streams (default schedule)
    h.estimate_ground_batch(big, mode=pwpp_hip.MODE_FRESH)
    for i in (0, 1, 63, 64, 65, 126, 127):
        assert_frame_equal(h, i, refs[i % 4], big[i].shape[0])
    counts = h.all_counts()
    for i in range(128):
        assert tuple(counts[i, :3]) == tuple(counts[i % 4, :3])


def test_bench_two_ranks_on_one_gpu():
    """bench.py's N > 1 path end to end (one process per rank under torch.distributed.run, per-rank Handle, sharded
    source frames, barrier, MAX-time / SUM-frames aggregation) with the only GPU this box has: both ranks on GPU 0,
    gloo instead of RCCL.  What it cannot show is RCCL over xGMI and 8 x 52 GB of workspaces: unmeasured on hardware
    until the driver's SCALE run."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, PWPP_BENCH_SHARE_DEVICE="1", PWPP_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")

    def run(frames, extra, bare=False):
        # bare: `python bench.py --gpus 2` as a plain process -- the way the driver starts --gpus 1 -- which must spawn its own ranks
        launcher = [] if bare else ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                                    "--master-port", str(port)]
        cmd = [sys.executable] + launcher + [os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                                             "--frames", str(frames), "--no-cpu-baseline", "--skip-latency"] + extra
        out = subprocess.run(cmd, env={k: v for k, v in env.items() if bare is False or k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")},
                             cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout  # rank 0 alone prints
        return json.loads(lines[0])

    d = run(192, ["--full"])  # (parity_check, reference_order and the self-checks are --full legs)
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["scaling"] == "weak"
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 2 * 192) < 1e-6 * 2 * 192  # whole-job frames per step / max time
    assert "cpu_baseline" not in d and d["config"]["frames_per_gpu"] == 192
    # per-GPU and aggregate (BASELINE.json configs[3]): every rank's own rate, in rank order; the aggregate is total frames
    # over the SLOWEST rank's time, so it cannot exceed the sum of the ranks' rates
    assert [g["rank"] for g in d["per_gpu"]] == [0, 1] and all(g["frames_per_s"] > 0 for g in d["per_gpu"])
    assert d["value"] <= sum(g["frames_per_s"] for g in d["per_gpu"]) * (1 + 1e-9)
    assert d["selfcheck"] is True and d["parity_check"]["iou"] == 1.0 and d["parity_check"]["frames"] == 7
    assert d["reference_order"]["ms_per_step"] > 0 and "ingest" not in d  # (the ingest leg is rank 0's at N = 1 only)
    assert d["dist"]["world_size"] == 2 and d["dist"]["backend"] == "gloo" and len(d["dist"]["devices"]) == 2
    assert d["dist"]["launcher"] == "torch.distributed.run" and len(d["dist"]["workspace_gb_per_rank"]) == 2
    # the bare form: no launcher around it, WORLD_SIZE unset -- bench.py re-runs itself as two ranks and still prints ONE line
    d = run(64, ["--skip-extras"], bare=True)
    assert d["n_gpus"] == 2 and d["config"]["frames_per_gpu"] == 64 and len(d["per_gpu"]) == 2
    assert d["dist"]["world_size"] == 2 and d["dist"]["launcher"].startswith("bench.py spawned")
    # the dense workload (configs[4]) through the same N > 1 path: 2 x 16 frames of ~486 k points, 36-sector CZM
    d = run(16, ["--workload", "dense", "--skip-extras"])
    assert d["n_gpus"] == 2 and d["config"]["frames_per_gpu"] == 16 and d["config"]["points_per_frame"] > 400000
    assert len(d["per_gpu"]) == 2 and "parity_check" not in d


def test_bench_plain_run_and_dumped_outputs(golden, tmp_path):
    """`bench.py --gpus 1` without --full prints the headline line and runs none of the legs outside the timed region; with
    --dump-outputs it writes the last timed step's results as float .npy files (at most 64 MB): the same files from two runs with
    the same arguments, the sampled frames' ground labels equal to the reference's masks of their source frames, and counts, labels
    and patch rows that agree with each other."""
    import json
    import subprocess
    import sys
    import pwpp_dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames, steps = 256, 3
    legs = {"parity_check", "synchronous", "exact_moments_off", "kernel_ms", "roofline", "latency", "reference_order", "ingest",
            "dense", "distinct", "streams", "cpu_baseline"}
    dumps = []
    for k in range(2):
        out_dir = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                              "--frames", str(frames), "--dump-outputs", str(out_dir)], cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"]
        assert abs(d["value"] * d["ms_per_step"] * 1e-3 - frames) < 1e-6 * frames
        assert not legs & set(d) and d["selfcheck"] is False
        a = {p.name[:-4]: np.load(p) for p in out_dir.glob("*.npy")}
        assert set(a) == {"counts", "state", "sample_frames", "labels", "normals", "centers"}
        assert all(v.dtype in (np.float32, np.float64) for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
        dumps.append(a)
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name], equal_nan=True), name
    a = dumps[0]
    counts, sample = a["counts"].astype(np.int64), a["sample_frames"].astype(np.int64)
    assert counts.shape == (frames, 6) and a["state"].shape == (frames, 9) and 0 < len(sample) <= 64
    # two batches in flight: step k ran batch k mod 2, whose buffers replay the six sources in rotation k mod 2
    which = pwpp_dist.shard_sources(6, frames, (steps - 1) % 2)
    at = 0
    for i in sample:
        n = int(counts[i, 0] + counts[i, 1] + counts[i, 5])
        lab = a["labels"][at:at + n]
        at += n
        assert (lab == 1).sum() == counts[i, 0] and (lab == 0).sum() == counts[i, 1] and (lab == -1).sum() == counts[i, 5]
        assert np.array_equal((lab == 1).astype(np.uint8), np.unpackbits(golden["f32/fresh/%d/ground_mask" % which[i]])[:n])
    assert at == len(a["labels"])
    assert a["normals"].shape == a["centers"].shape == (int(counts[sample, 2].sum()), 3)


def test_bench_eight_ranks_on_one_gpu():
    """the driver's first `bench.py --gpus 8` cannot be rehearsed on eight GPUs here -- so it is rehearsed as EIGHT
    ranks on the one GPU (gloo, every rank on device 0), started bare the way the driver starts it: one JSON line, eight per-GPU
    rates, eight workspaces, world size 8; the headline workload and the stateful-streams workload (stream g on rank g mod 8).
    RCCL over xGMI stays unmeasured on hardware."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(PWPP_BENCH_SHARE_DEVICE="1", PWPP_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for workload, frames in (("kitti", 32), ("streams", 4)):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1", "--frames", str(frames),
                              "--workload", workload, "--no-cpu-baseline", "--skip-latency", "--skip-extras"], env=env, cwd=root,
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout
        d = json.loads(lines[0])
        assert d["n_gpus"] == 8 and d["dist"]["world_size"] == 8 and d["dist"]["backend"] == "gloo"
        assert [g["rank"] for g in d["per_gpu"]] == list(range(8)) and all(g["frames_per_s"] > 0 for g in d["per_gpu"])
        assert len(d["dist"]["workspace_gb_per_rank"]) == 8 and len(d["dist"]["devices"]) == 8
        assert d["dist"]["launcher"].startswith("bench.py spawned")
        assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 8 * frames) < 1e-6 * 8 * frames
        if workload == "streams":
            # ranks 0 and 6 hold streams that start on the same source frame (g mod 6): the same adaptive state after the same frames
            hts = d["sensor_height_of_each_ranks_first_stream"]
            assert len(hts) == 8 and hts[0] == hts[6] and hts[1] == hts[7] and hts[0] != hts[1]


def test_precleared_counters_under_changing_call_shapes(kitti, oracle):
    """The counters a call starts from exist twice: a call's K5 zeroes the other copy for the next call, which then needs no
    clearing kernel -- but only if that call has the same shape (frames, binning path, allocations).  One handle through
    calls whose shape keeps changing: single fresh frames back to back (the pre-cleared path), batches of other sizes in
    between, stream mode, a trimmed workspace, the two-pass path forced, a segment overflow with its redo, a frame that needs
    the serial fix-up -- every result against the oracle."""
    h = pwpp_hip.Handle()
    h.set_option("debug_flags", 64)  # every call that skips k_clear first reads its counters back: all zero, or PWPP_E_STATE
    refs = [ol.Estimator(oracle, arith=ol.ARITH_FXP).run(k) for k in kitti]

    def fresh(idx):
        h.estimate_ground_batch([kitti[i] for i in idx], mode=pwpp_hip.MODE_FRESH)
        for j, i in enumerate(idx):
            assert_frame_equal(h, j, refs[i], kitti[i].shape[0])

    for i in (0, 1, 2):
        fresh([i])                      # same shape three times: the second and third run without k_clear
    fresh([3, 4, 5, 0, 1, 2, 3, 4])     # other frame count: cleared by the kernel again ...
    fresh([5, 4, 3, 2, 1, 0, 5, 4])     # ... and pre-cleared
    fresh([2])
    h.trim_workspace()
    fresh([1])
    fresh([1])
    h.set_option("one_pass", 0)         # two-pass binning: three slabs of counters instead of one
    fresh([4])
    fresh([4])
    h.set_option("one_pass", 1)
    fresh([0])
    fresh([0])
    # a stateful stream on the same handle in between (its own sequential oracle)
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for i in (0, 1):
        h.estimate_ground(kitti[i])
        assert_frame_equal(h, 0, est.run(kitti[i]), kitti[i].shape[0], state_index=0)
    fresh([3])
    # a cloud that overflows its one-pass segments (70 % of the points in one wedge): redo on the other path, then on
    rng = np.random.default_rng(9)
    wedge = kitti[2].copy()
    sel = rng.random(wedge.shape[0]) < 0.7
    r = np.hypot(wedge[sel, 0], wedge[sel, 1])
    a = rng.uniform(0.1, 0.27, sel.sum())
    wedge[sel, 0] = (r * np.cos(a)).astype(np.float32)
    wedge[sel, 1] = (r * np.sin(a)).astype(np.float32)
    wref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(wedge)
    for _ in range(2):
        h.estimate_ground_batch([wedge], mode=pwpp_hip.MODE_FRESH)
        assert_frame_equal(h, 0, wref, wedge.shape[0])
        fresh([5])
    # a frame with a patch that starts from the plane fitted before it (k_fit_fixup runs K5 a second time for it)
    odd = kitti[1].copy()
    odd[:40, 2] = -np.inf
    oref = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(odd)
    for _ in range(2):
        h.estimate_ground_batch([odd], mode=pwpp_hip.MODE_FRESH)
        assert_frame_equal(h, 0, oref, odd.shape[0])
    fresh([0])


def test_rccl_code_path_with_a_single_rank_group():
    """What can be run of bench.py's RCCL plumbing on a one-GPU box: a process group of ONE rank on backend "nccl" (= RCCL)
    with device_id, the barrier that names the rank's device, the MAX / SUM all-reduces and the all-gather of the per-GPU
    rates (tools/rccl_single_rank.py, its own process).  Ranks 1-7 and xGMI stay unmeasured until the driver's SCALE run."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "rccl_single_rank.py")], cwd=root, env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert "aggregate (1.5, 7)" in out.stdout and "gather [3.25]" in out.stdout and "rccl single-rank ok" in out.stdout


def test_pipe_in_stream_mode(kitti, oracle):
    """pwpp_pipe_submit with PWPP_MODE_STREAMS (round 6): two groups of stateful streams, handle g of the pipe owns group g, submit k
    carries the next frames of group k mod 2 -- batches in flight for the reference's real use (one long-lived object per sensor,
    demo_sequential.cpp:54-67).  Every stream against its own sequential run of the restatement: lists, planes, state, histories.
    Small groups (3 streams: the latency plan) and groups of 70 (the throughput kernels with stream state)."""
    import torch
    dev = torch.device("cuda", 0)
    bufs = [torch.from_numpy(f).to(dev) for f in kitti]
    for S, T in ((3, 4), (70, 3)):
        pipe = pwpp_hip.Pipe(depth=2)
        pipe.set_num_streams(S)
        ests = [[ol.Estimator(oracle, arith=ol.ARITH_FXP) for _ in range(S)] for _ in range(2)]
        src = lambda g, s, t: (5 * g + s + t) % 6
        batches = [[pipe.handle(g).make_device_batch([bufs[src(g, s, t)].data_ptr() for s in range(S)], [kitti[src(g, s, t)].shape[0] for s in range(S)])
                    for t in range(T)] for g in range(2)]
        with pytest.raises(pwpp_hip.PwppError, match="streams"):  # a group larger than the handle's stream count
            pipe.submit_device_batch(pipe.handle(0).make_device_batch([bufs[0].data_ptr()] * (S + 1), [kitti[0].shape[0]] * (S + 1)), mode=pwpp_hip.MODE_STREAMS)
        holders = []
        for k in range(2 * T):  # all submits first: two lock-steps in flight
            holders.append(pipe.submit_device_batch(batches[k % 2][k // 2], mode=pwpp_hip.MODE_STREAMS))
            if k >= 1:  # the batch submitted one step ago is complete once its handle is synchronised; check it before it comes round again
                g, t = (k - 1) % 2, (k - 1) // 2
                hv = holders[k - 1]
                hv.synchronize()
                for s in (range(S) if S <= 8 else (0, 1, S // 2, S - 1)):
                    while len(getattr(ests[g][s], "_done", [])) <= t:
                        done = getattr(ests[g][s], "_done", [])
                        done.append(ests[g][s].run(kitti[src(g, s, len(done))]))
                        ests[g][s]._done = done
                    assert_frame_equal(hv, s, ests[g][s]._done[t], kitti[src(g, s, t)].shape[0], state_index=s)
        pipe.drain()
        assert holders[0]._h.value == holders[2]._h.value != holders[1]._h.value
        pipe.close()


def test_overflow_arena_moves_parts_on_the_device(kitti, oracle):
    """Round 6: a part's segment holds ~1.125 x its largest count so far, and a frame's OVERFLOW ARENA takes what does not fit -- the
    binning kernel spills the points with {part, rank} tags, k_czm_scan moves every overgrown part into the arena as a whole (pwpp_dev.h).
    Two frames of 72 get 40 % more points in one sector than the handle has ever seen there: ~25 parts each outgrow their segments,
    nothing is binned again by the host, and both frames (their neighbours too) are the oracle's bit for bit -- lists, patch records,
    planes, state.  The same batches with the arena switched off (debug_flags 2048) do go back to the host: the overflow was real.
    Then through the overlap schedule (two frame ranges) and as stateful streams."""
    rng = np.random.default_rng(11)

    def denser(src, lo, hi, factor):
        a = np.arctan2(src[:, 1], src[:, 0])
        sel = np.where((a > lo) & (a < hi))[0]
        extra = src[rng.choice(sel, int(len(sel) * factor), replace=True)].copy()
        extra[:, :3] += rng.normal(0.0, 0.004, (len(extra), 3)).astype(np.float32)
        return np.ascontiguousarray(np.concatenate([src, extra]).astype(np.float32))

    est = lambda p: ol.Estimator(oracle, arith=ol.ARITH_FXP).run(p)
    refs = [est(k) for k in kitti]
    F = 72
    base = [kitti[i % 6] for i in range(F)]
    d0, d1 = denser(kitti[0], 0.3, 0.6, 0.4), denser(kitti[3], -2.2, -1.9, 0.4)
    odd = list(base)
    odd[10], odd[40] = d0, d1
    special = {10: est(d0), 40: est(d1)}
    for arena in (True, False):
        h = pwpp_hip.Handle()
        if not arena:
            h.set_option("debug_flags", 2048)
        h.estimate_ground_batch(base, mode=pwpp_hip.MODE_FRESH)
        assert h.redo_stats() == (F, 0)
        h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
        if arena:
            assert h.redo_stats() == (2 * F, 0), h.redo_stats()
        else:
            assert h.redo_stats()[0] == 2 * F and h.redo_stats()[1] >= 1, h.redo_stats()  # (frame 10 for sure; frame 40's sector is sparser)
        for i in (9, 10, 11, 39, 40, 41, 0, F - 1):
            assert_frame_equal(h, i, special.get(i, refs[i % 6]), odd[i].shape[0])
        if arena:  # the moved parts' true counts sized the table: the same batch fits its segments now, and the results stand
            h.estimate_ground_batch(odd, mode=pwpp_hip.MODE_FRESH)
            assert h.redo_stats() == (3 * F, 0)
            for i in (10, 40):
                assert_frame_equal(h, i, special[i], odd[i].shape[0])
    # two frame ranges on the handle's streams (150 frames), the dense frames in different ranges; reference-ordered lists
    F2 = 150
    base2 = [kitti[i % 6] for i in range(F2)]
    odd2 = list(base2)
    odd2[5], odd2[140] = d0, d1
    for ordered in (False, True):
        h = pwpp_hip.Handle()
        h.set_output_order(ordered)
        h.estimate_ground_batch(base2, mode=pwpp_hip.MODE_FRESH)
        h.estimate_ground_batch(odd2, mode=pwpp_hip.MODE_FRESH)
        assert h.redo_stats() == (2 * F2, 0)
        for i, r in ((5, special[10]), (140, special[40]), (4, refs[4 % 6]), (141, refs[141 % 6])):
            assert_frame_equal(h, i, r, odd2[i].shape[0], check_state=False)
            if ordered:
                assert np.array_equal(odd2[i][h.ground_indices(i), 2], odd2[i][r.ground_idx, 2])
    # a PSEUDO-bin outgrows its segment (2 500 more returns beyond max_range than any frame before: indices only are moved), and a batch
    # of 24 frames (arena on, the small-batch variants of K5 / K6)
    far = kitti[1][np.hypot(kitti[1][:, 0], kitti[1][:, 1]) > 40.0]
    extra = far[rng.choice(len(far), 2500, replace=True)].copy()
    extra[:, :2] *= 2.6  # 104 m and more: out of range
    d2 = np.ascontiguousarray(np.concatenate([kitti[1], extra]).astype(np.float32))
    r2 = est(d2)
    assert len(r2.nonground_idx) >= len(refs[1].nonground_idx) + 2500
    h = pwpp_hip.Handle()
    small = [kitti[i % 6] for i in range(24)]
    h.estimate_ground_batch(small, mode=pwpp_hip.MODE_FRESH)
    odd3 = list(small)
    odd3[7], odd3[20] = d2, d0
    h.estimate_ground_batch(odd3, mode=pwpp_hip.MODE_FRESH)
    assert h.redo_stats() == (48, 0) and h.arena_stats()[0] == 2, (h.redo_stats(), h.arena_stats())
    for i, r in ((7, r2), (20, special[10]), (6, refs[0]), (8, refs[2]), (23, refs[5])):
        assert_frame_equal(h, i, r, odd3[i].shape[0])
    # stateful streams: 70 in lock-step, stream 33 meets the dense frame at step 2 -- no state restore, no redo
    S = 70
    hs = pwpp_hip.Handle()
    hs.set_num_streams(S)
    e33, e34 = ol.Estimator(oracle, arith=ol.ARITH_FXP), ol.Estimator(oracle, arith=ol.ARITH_FXP)
    for t in range(4):
        frames = [kitti[(s + t) % 6] for s in range(S)]
        if t == 2:
            frames[33] = d0
        hs.estimate_ground_batch(frames, mode=pwpp_hip.MODE_STREAMS)
        assert_frame_equal(hs, 33, e33.run(frames[33]), frames[33].shape[0], state_index=33)
        assert_frame_equal(hs, 34, e34.run(frames[34]), frames[34].shape[0], state_index=34)
    assert hs.redo_stats()[1] == 0


def test_exact_moments_option(kitti, oracle):
    """The width of the plane-fit sums is a handle option: exact_moments = 1 (default; contract v4, a 2^-30 m grid on which the reference's
    floats lie) or 0 (rounds 3-5's 2^-21 m grid, faster).  Either way the HIP path is its restatement bit for bit -- single frames (the
    four-waves / hybrid kernels), a batch of 70 (the throughput kernels), a stateful stream -- and switching back and forth on one
    handle changes nothing else.  The two grids themselves differ by a few float ulps in the planes (and, off KITTI, by an index now
    and then: tools/parity_statistics.py)."""
    h = pwpp_hip.Handle()
    assert h._L.pwpp_get_fxp_shift(h._h) == 30
    for value, arith, shift in ((0, ol.ARITH_FXP21, 21), (1, ol.ARITH_FXP, 30), (0, ol.ARITH_FXP21, 21)):
        h.set_option("exact_moments", value)
        assert h._L.pwpp_get_fxp_shift(h._h) == shift
        refs = [ol.Estimator(oracle, arith=arith).run(k) for k in kitti]
        for k in (0, 2, 5):
            h.estimate_ground_batch([kitti[k]], mode=pwpp_hip.MODE_FRESH)
            assert_frame_equal(h, 0, refs[k], kitti[k].shape[0])
        frames = [kitti[i % 6] for i in range(70)]
        h.estimate_ground_batch(frames, mode=pwpp_hip.MODE_FRESH)
        for i in (0, 1, 33, 69):
            assert_frame_equal(h, i, refs[i % 6], frames[i].shape[0], check_state=False)
    hs = pwpp_hip.Handle()
    hs.set_option("exact_moments", 0)
    est = ol.Estimator(oracle, arith=ol.ARITH_FXP21)
    for t in range(5):
        hs.estimate_ground(kitti[t % 6])
        assert_frame_equal(hs, 0, est.run(kitti[t % 6]), kitti[t % 6].shape[0], state_index=0)
    with pytest.raises(pwpp_hip.PwppError):
        hs.set_option("exact_moments", 2)
    a = ol.Estimator(oracle, arith=ol.ARITH_FXP).run(kitti[0])
    b = ol.Estimator(oracle, arith=ol.ARITH_FXP21).run(kitti[0])
    assert np.array_equal(np.sort(a.ground_idx), np.sort(b.ground_idx)) and not np.array_equal(a.normals, b.normals)
    assert np.abs(a.normals - b.normals).max() < 1e-4
