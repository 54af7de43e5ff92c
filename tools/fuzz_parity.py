#!/usr/bin/env python3
"""Randomised differential test of the HIP path against the CPU restatement (oracle/, fixed-point flavour): random
parameter sets inside what pwpp_create accepts, random synthetic clouds with adversarial additions (walls next to the
sensor, slopes, +-inf / huge heights, duplicates, outliers), random bin splits, fit plans, fresh batches and stateful
sequences -- every case must be bit-identical (index sets, patch records, planes, adaptive state, histories).

usage (on the GPU box):  python tools/fuzz_parity.py [cases] [first_seed]
A failing case prints its seed; `python tools/fuzz_parity.py 1 <seed>` reproduces it.
"""
import os
import sys
import time
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "patchwork-plusplus_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import oracle_lib as ol  # noqa: E402
import pwpp_hip  # noqa: E402
import pwpp_synth  # noqa: E402
from test_gpu_parity import assert_frame_equal, to_oracle_params  # noqa: E402

LAST = ""
ARITH = ol.ARITH_FXP
PLANS = ["", "", "", "W16:1023,W64.2:65535", "W16.16:1023,S64:65535", "S16:255,S64:65535", "B64:65535", "S8:63,S16:255,S32:1023,S64:4095",
         "W16.32:511,W64.4:65535", "H64:255", "S16:100", "W16:255,W64.8:65535"]


def random_params(rng, p=None):
    """Draws a parameter set into `p` (default: pwpp_hip.default_params(); any structure with the same field names will do,
    e.g. the oracle's, where the HIP library is not there)."""
    p = pwpp_hip.default_params() if p is None else p
    if rng.random() < 0.3:
        p.enable_RNR = int(rng.integers(0, 2))
    if rng.random() < 0.3:
        p.enable_RVPF = int(rng.integers(0, 2))
    if rng.random() < 0.3:
        p.enable_TGR = int(rng.integers(0, 2))
    if rng.random() < 0.5:
        p.num_iter = int(rng.integers(1, 6))
    if rng.random() < 0.5:
        p.num_lpr = int(rng.choice([3, 5, 10, 20, 40, 64, 100, 200]))
    if rng.random() < 0.5:
        p.num_min_pts = int(rng.choice([0, 0, 1, 3, 5, 10, 20, 50, 200]))  # (0: empty bins are processed and report the plane fitted last)
    if rng.random() < 0.5:
        p.th_seeds = float(rng.choice([0.1, 0.125, 0.2, 0.3, 0.5]))
        p.th_dist = float(rng.choice([0.1, 0.125, 0.2, 0.3]))
    if rng.random() < 0.5:
        p.th_seeds_v = float(rng.choice([0.1, 0.25, 0.4, 0.8]))
        p.th_dist_v = float(rng.choice([0.05, 0.1, 0.3]))
    if rng.random() < 0.4:
        p.uprightness_thr = float(rng.choice([0.5, 0.707, 0.9, 0.99, 0.9999]))
    if rng.random() < 0.4:
        p.sensor_height = float(rng.uniform(0.8, 2.5))
    if rng.random() < 0.3:
        p.adaptive_seed_selection_margin = float(rng.uniform(-1.5, -0.6))
    if rng.random() < 0.4:
        p.min_range = float(rng.uniform(0.5, 4.0))
        p.max_range = float(rng.uniform(30.0, 150.0))
    if rng.random() < 0.4:
        for k in range(4):
            p.num_sectors_each_zone[k] = int(rng.choice([4, 8, 16, 32, 36, 54, 64]))
            p.num_rings_each_zone[k] = int(rng.integers(1, 6))
    if rng.random() < 0.3:
        p.num_rings_of_interest = int(rng.integers(1, 5))
    if rng.random() < 0.2:
        p.max_flatness_storage = int(rng.integers(3, 40))
        p.max_elevation_storage = int(rng.integers(3, 40))
    return p


ODD_HEIGHTS = True


def random_cloud(rng, sensor_height):
    beams = int(rng.choice([16, 32, 48, 64]))
    steps = int(rng.choice([400, 900, 1500, 2000]))
    pts = pwpp_synth.make_cloud(int(rng.integers(0, 1 << 30)), beams=beams, azimuth_steps=steps, sensor_height=sensor_height,
                                n_boxes=int(rng.integers(0, 120)), undulation=float(rng.choice([0.0, 0.15, 0.6, 1.5])),
                                reflect_frac=float(rng.choice([0.0, 0.02, 0.1])), range_noise=float(rng.choice([0.0, 0.02, 0.1])))
    extra = []
    if rng.random() < 0.5:  # walls near the sensor, from below the ground to well above it
        k = int(rng.integers(200, 4000))
        w = np.zeros((k, 4), np.float32)
        ang = np.repeat(rng.uniform(0, 2 * np.pi, 8), (k + 7) // 8)[:k]
        rad = np.repeat(rng.uniform(3.0, 15.0, 8), (k + 7) // 8)[:k] + rng.normal(0, 0.01, k)
        w[:, 0], w[:, 1] = rad * np.cos(ang), rad * np.sin(ang)
        w[:, 2] = rng.uniform(-sensor_height - 0.5, 2.0, k)
        w[:, 3] = rng.uniform(0, 1, k)
        extra.append(w)
    if rng.random() < 0.4:  # a steep ramp in one direction
        k = int(rng.integers(500, 5000))
        r = np.zeros((k, 4), np.float32)
        r[:, 0] = rng.uniform(3, 40, k)
        r[:, 1] = rng.uniform(-5, 5, k)
        r[:, 2] = -sensor_height + float(rng.uniform(-0.3, 0.3)) * r[:, 0] + rng.normal(0, 0.02, k)
        r[:, 3] = 0.5
        extra.append(r)
    if rng.random() < 0.4 and ODD_HEIGHTS and not os.environ.get("FUZZ_NO_ODD"):  # odd heights and duplicates
        k = int(rng.integers(1, 30))
        o = pts[rng.integers(0, len(pts), k)].copy()
        # (-inf as the lowest height of a bin, or a lone 1e30 with num_min_pts <= 1, leaves a patch's first seed set empty:
        # it then starts from the plane the reference object fitted last -- the serial fix-up path, pwpp_fit.hip)
        o[:, 2] = rng.choice(np.array([np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 100.0, -100.0, 3e38, -3e38], np.float32), k)
        extra.append(o)
        extra.append(pts[rng.integers(0, len(pts), int(rng.integers(1, 200)))].copy())
    if rng.random() < 0.3:
        pts = pwpp_synth.add_edge_cases(pts, int(rng.integers(0, 1000)))
    if rng.random() < 0.3:  # a blind sector (with num_min_pts = 0 its bins report the plane of the bin, or frame, before)
        a0 = float(rng.uniform(0, 360))
        ang = np.degrees(np.arctan2(pts[:, 1], pts[:, 0])) % 360.0
        pts = pts[((ang - a0) % 360.0) > float(rng.uniform(20, 200))]
    if extra:
        pts = np.concatenate([pts] + extra).astype(np.float32)
        rng.shuffle(pts, axis=0)
    if rng.random() < 0.15:
        pts = np.ascontiguousarray(pts[:, :3])
    return np.ascontiguousarray(pts)


def one_case(seed, oracle):
    rng = np.random.default_rng(seed)
    p = random_params(rng)
    global ODD_HEIGHTS
    ODD_HEIGHTS = True
    h = pwpp_hip.Handle(p)
    plan = PLANS[int(rng.integers(0, len(PLANS)))]
    if plan:
        h.set_option("fit_plan", plan)
    h.set_option("hi_split", float(rng.choice([-1.0, 0.0, 0.1, 0.3, 0.6, 1.0, 2.5, 1e30])))
    h.set_option("hi_split_zones", int(rng.integers(0, 5)))
    if os.environ.get("FUZZ_NO_SPLIT"):
        h.set_option("hi_split_zones", 0)
    if os.environ.get("FUZZ_PLAN") is not None:
        h.set_option("fit_plan", os.environ["FUZZ_PLAN"])
    opm = rng.random() < 0.25
    if opm:
        h.set_option("one_pass_min_frames", 1)
        if rng.random() < 0.5:
            h.set_option("one_pass_scale", float(rng.choice([0.02, 0.2, 1.0])))  # segments far too small: overflow, exact redo
    global ARITH
    ARITH = ol.ARITH_FXP  # contract v4 (the default); one case in six runs rounds 3-5's narrow grid behind its option
    if rng.random() < 0.17:
        h.set_option("exact_moments", 0)
        ARITH = ol.ARITH_FXP21
    rng2 = np.random.default_rng(seed + 10 ** 9)  # (a generator of its own: the cases of earlier records stay what they were)
    h.set_option("split_k5", int(rng2.choice([1, 1, 0, 2])))   # K5 of a few stateful streams in one launch / two / the second behind the lists
    ordered = rng.random() < 0.2   # the reference's own order inside the lists (ties among equal heights aside)
    h.set_output_order(ordered)
    fortran = rng.random() < 0.2   # column-major matrices (Eigen's storage)
    mode = rng.random()
    if os.environ.get("FUZZ_BIG"):  # only the big-batch mode
        mode = 0.99
    global LAST
    LAST = "plan '%s' one_pass_min_frames=1: %s ordered %s fortran %s mode %.2f" % (plan, opm, ordered, fortran, mode)

    def check(i, ref, pts, **kw):
        assert_frame_equal(h, i, ref, pts.shape[0], **kw)
        if ordered:
            z = pts[:, 2]
            for mine, theirs in ((h.ground_indices(i), ref.ground_idx), (h.nonground_indices(i), ref.nonground_idx)):
                assert np.array_equal(z[mine], z[np.asarray(theirs)], equal_nan=True), "the z sequence differs from the reference's"

    def lay(c):
        return np.asfortranarray(c) if fortran else c
    if mode >= 0.94:  # (round 5) a BIG fresh batch: the kernels only batches above 64 / 128 frames run (list kernel with one wave per
        # bin and its long-list launch, K5's throughput variant, the XCD-dealt binning, the overlap schedule), on a few distinct clouds replayed
        distinct = [random_cloud(rng, p.sensor_height) for _ in range(int(rng.integers(2, 6)))]
        if len({f.shape[1] for f in distinct}) > 1:
            distinct = [np.ascontiguousarray(f[:, :3]) for f in distinct]
        refs = [ol.Estimator(oracle, to_oracle_params(p), arith=ARITH).run(f) for f in distinct]
        nfr = int(rng.choice([65, 72, 100, 129, 136, 160]))
        pick = [int(rng.integers(0, len(distinct))) for _ in range(nfr)]
        seen = max(1, len(distinct) // 2)
        for rep in range(3):  # (the first call only holds half of the clouds: the second meets bins fuller than any the handle has seen --
            # overflow arena, parts moved on the device, or a redo; the third knows the bins with long lists)
            if rep == 0:
                pick0 = [k % seen for k in pick]
                h.estimate_ground_batch([lay(distinct[k]) for k in pick0], mode=pwpp_hip.MODE_FRESH)
                for i in (0, nfr // 2, nfr - 1):
                    check(i, refs[pick0[i]], distinct[pick0[i]], check_state=False)
                continue
            h.estimate_ground_batch([lay(distinct[k]) for k in pick], mode=pwpp_hip.MODE_FRESH)
            for i in sorted(set(int(x) for x in rng.integers(0, nfr, 24)) | {0, nfr - 1}):
                check(i, refs[pick[i]], distinct[pick[i]], check_state=False)
        return "big batch of %d" % nfr
    if mode < 0.45:  # a fresh batch
        frames = [random_cloud(rng, p.sensor_height) for _ in range(int(rng.integers(1, 7)))]
        if len({f.shape[1] for f in frames}) > 1:
            frames = [np.ascontiguousarray(f[:, :3]) for f in frames]
        h.estimate_ground_batch([lay(f) for f in frames], mode=pwpp_hip.MODE_FRESH)
        for i, pts in enumerate(frames):
            check(i, ol.Estimator(oracle, to_oracle_params(p), arith=ARITH).run(pts), pts)
        return "batch of %d" % len(frames)
    if mode < 0.78:  # one stateful stream, frame after frame
        est = ol.Estimator(oracle, to_oracle_params(p), arith=ARITH)
        n = int(rng.integers(2, 6))
        for _ in range(n):
            pts = random_cloud(rng, p.sensor_height)
            h.estimate_ground(lay(pts))
            check(0, est.run(pts), pts, state_index=0)
        return "sequence of %d" % n
    streams = int(rng.integers(2, 5))  # several streams in lock step
    h.set_num_streams(streams)
    ests = [ol.Estimator(oracle, to_oracle_params(p), arith=ARITH) for _ in range(streams)]
    cols = 3 if rng.random() < 0.2 else 4
    for _ in range(int(rng.integers(2, 4))):
        frames = [random_cloud(rng, p.sensor_height) for _ in range(streams)]
        if cols == 3 or len({f.shape[1] for f in frames}) > 1:  # (one column count per call)
            frames = [np.ascontiguousarray(f[:, :3]) for f in frames]
        h.estimate_ground_batch([lay(f) for f in frames], mode=pwpp_hip.MODE_STREAMS)
        for i, pts in enumerate(frames):
            check(i, ests[i].run(pts), pts)
    return "%d streams" % streams


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    ol.build()
    oracle = ol.restatement()
    failed = []
    t0 = time.time()
    for seed in range(first, first + cases):
        try:
            what = one_case(seed, oracle)
            if cases <= 20:
                print("seed %d ok (%s)" % (seed, what))
        except Exception as e:  # keep going: the list of failing seeds is the result
            failed.append(seed)
            print("seed %d FAILED (%s): %s" % (seed, LAST, str(e)[:300]))
            if len(failed) <= 3:
                traceback.print_exc()
    print("%d cases, %d failed %s, %.0f s" % (cases, len(failed), failed[:40], time.time() - t0))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
