"""What the correlative scan match (pwpp_match_obstacles, pwpp_match_grid) costs on one MI355X (profiles/scan_match_cost.txt), and
the A/B of the option "match_path": "1" the yardstick, every map read from global memory; "2" the rectangle of the map in reach
of a (frame, candidate) staged in LDS.  What "0", the default, means (kMatchDefaultStage in csrc/pwpp_match.hip) follows from it.

  * `frames` replayed KITTI frames in device memory on 256 x 256 cells of 0.5 m, band [0.2, 2.5] m, min_count 1, origin {0, 0},
    max_range 40, matched against maps of 256 x 256 cells of 0.5 m with 21 yaw candidates per frame (a set per frame: the frame's
    displaced prior first, then +-1 .. +-10 steps of 0.01 rad) and a window of +-10 cells, 441 shifts, for
      (a) `frames` maps, frame i against map i      (b) one map for all frames      (c) 16 maps, frame i against map i % 16
    on both paths, and path 1 a second time as its own A/A twin.  The maps are what pwpp_fuse_obstacles made of the same frames under the true poses (fused once per case, not
    timed); the prior of frame i is its true pose turned by -1 step and moved by (+2, -1) cells, so the true answer of case (a) is
    candidate 1, shift (-2, +1): the tool counts the frames that return it.  best is a device array, scores are not asked for, the
    per-frame bytes stay in the handle's buffer.
  * The yardstick: pwpp_visibility_obstacles alone on the same handle and grid, in the same rounds -- the match's own cost is the
    difference -- and pwpp_match_grid alone on the device images a visibility call left.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), so that a drift of the
  clocks hits every variant alike, and the order is reversed in every other round, so that no variant always follows the same one.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host
  clock and divided by `reps`.  The whole set is run `runs` times in this process (fresh handles each time): a difference
  between the two paths counts where it exceeds both the spread BETWEEN runs and the distance of path 1 from its A/A twin.

    python tools/scan_match_cost.py [--frames 1024] [--steps 6] [--warmup 1] [--reps 2] [--runs 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "patchwork-plusplus_amd/python", "tools", ""):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libpwpp_hip: see tests/conftest.py)

import bench  # noqa: E402
import pwpp_hip  # noqa: E402
from point_records_cost import device_batch  # noqa: E402

NX = NY = 256
CELL = 0.5
BAND = (0.2, 2.5)
MAX_RANGE = 40
N_CANDIDATES, YAW_STEP, WINDOW = 21, 0.01, 10
TRUTH = (1, -2, 1)  # candidate, sx, sy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_match_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    x0 = y0 = -0.5 * NX * CELL
    per = NX * NY
    fmap = pwpp_hip.FusionMap(x0, y0, CELL, NX, NY, 40, 20, -200, 350, 60, -40)
    # the vehicle drives a circle of 8 m radius: yaw and translation change with every frame
    yaw = 0.005 * np.arange(F)
    poses = np.stack([np.cos(yaw), -np.sin(yaw), 8.0 * np.sin(yaw), np.sin(yaw), np.cos(yaw), 8.0 * (1.0 - np.cos(yaw))], axis=1)
    prior_yaw = yaw - YAW_STEP
    priors = np.stack([np.cos(prior_yaw), -np.sin(prior_yaw), poses[:, 2] + 2 * CELL, np.sin(prior_yaw), np.cos(prior_yaw), poses[:, 5] - CELL], axis=1)
    cand = np.stack([pwpp_hip.yaw_candidates(p, YAW_STEP, N_CANDIDATES) for p in priors])
    cases = [("(a) %d maps, frame i against map i" % F, F, None), ("(b) one map for all %d frames" % F, 1, None),
             ("(c) 16 maps, frame i against map i % 16", 16, np.arange(F, dtype=np.int32) % 16)]
    d_first, d_count = (torch.empty(F * per, dtype=torch.int32, device="cuda") for _ in range(2))
    d_occ = torch.empty(F * per, dtype=torch.int8, device="cuda")
    d_maps = [torch.zeros(n_maps * per, dtype=torch.int16, device="cuda") for _, n_maps, _ in cases]
    d_best = torch.zeros(3 * F, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    medians, head, labels = [], False, {}
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()
        for (_, n_maps, mof), d_map in zip(cases, d_maps):  # the maps: the frames fused under their true poses
            h.fuse_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], poses, fmap, n_maps, 0, d_map.data_ptr(), 0, 0, (0.0, 0.0), 1, MAX_RANGE, 0, F, mof)
        h.synchronize()

        def visibility():
            return timed(lambda: h.visibility_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], (0.0, 0.0), 1, MAX_RANGE, d_first.data_ptr(),
                                                               d_occ.data_ptr(), d_count.data_ptr(), 0, F), h.synchronize)

        def obstacles(n_maps, mof, d_map, path):
            def go():
                h.set_option("match_path", path)
                return timed(lambda: h.match_obstacles_device(x0, y0, CELL, NX, NY, BAND[0], BAND[1], cand, fmap, n_maps, d_map.data_ptr(), WINDOW, WINDOW,
                                                              d_best.data_ptr(), 0, 0, (0.0, 0.0), 1, MAX_RANGE, 0, F, mof), h.synchronize)
            return go

        def grid(n_maps, mof, d_map, path):
            def go():
                h.set_option("match_path", path)
                return timed(lambda: h.match_grid_device((x0, y0, CELL), NX, NY, F, d_occ.data_ptr(), cand, fmap, n_maps, d_map.data_ptr(), WINDOW, WINDOW,
                                                         d_best.data_ptr(), 0, mof), h.synchronize)
            return go

        visibility()  # (d_occ holds the frames' bytes from here on: what pwpp_match_grid reads)
        variants = {}  # key -> (name, measurement); keys: ("obstacles" | "grid", case, path), path "1 again": the A/A twin of path 1
        for what, make in (("obstacles", obstacles), ("grid", grid)):
            for ci, ((name, n_maps, mof), d_map) in enumerate(zip(cases, d_maps)):
                for path in (1, 2) + (("1 again",) if what == "grid" else ()):
                    label = "pwpp_match_%-9s %s, path %s" % (what, name, path)
                    variants[(what, ci, path)] = (label, make(n_maps, mof, d_map, 1 if path == "1 again" else path))
        variants["visibility"] = ("pwpp_visibility_obstacles (first, occupancy, count) alone", visibility)
        keys = list(variants)
        t = {k: [] for k in keys}
        for r in range(a.warmup + a.steps):
            for k in (keys if r % 2 == 0 else keys[::-1]):  # the order turns round with every round: no variant always follows the same one
                v = variants[k][1]()
                if r >= a.warmup:
                    t[k].append(v)
        if not head:
            head = True
            out("scan_match_cost: %s, %d frames, %d x %d cells of %.1f m, band [%.1f, %.1f] m, min_count 1, origin {0, 0}, max_range %d, %s"
                % (kind, F, NX, NY, CELL, BAND[0], BAND[1], MAX_RANGE, torch.cuda.get_device_name(0)))
            out("maps of %d x %d cells of %.1f m fused from the same frames; %d candidates per frame in steps of %.2f rad, window +-%d cells: %d shifts"
                % (NX, NY, CELL, N_CANDIDATES, YAW_STEP, WINDOW, (2 * WINDOW + 1) ** 2))
            for ci, (name, n_maps, mof) in enumerate(cases):
                variants[("grid", ci, 1)][1]()
                rows = np.frombuffer(d_best.cpu().numpy().tobytes(), pwpp_hip.MATCH_BEST_DTYPE)
                hit = int(((rows["candidate"] == TRUTH[0]) & (rows["sx"] == TRUTH[1]) & (rows["sy"] == TRUTH[2])).sum())
                out("  %s: %.0f occupied cells per frame (min %d, max %d); %d of %d frames return candidate %d, shift (%d, %d)"
                    % ((name, rows["cells"].mean(), rows["cells"].min(), rows["cells"].max(), hit, F) + TRUTH))
            out("path 1: every map read from global memory; path 2: the rectangle of the map in reach staged in LDS; path 1 again: path 1 a")
            out("second time in every round, the A/A twin whose distance from path 1 is what the method cannot resolve")
            out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds after %d warm-up rounds,"
                % (a.reps, a.steps, a.warmup))
            out("the order of the variants reversed in every other round; %d runs of the whole set, each with a fresh handle and batch" % a.runs)
            out()
        medians.append({k: float(np.median(t[k])) for k in keys})
        medians[-1]["batch"] = batch_us
        labels = {k: variants[k][0] for k in keys}
        labels["batch"] = "the batch's own pwpp_get_time_us"
        out("run %d (min .. max of the rounds in brackets):" % run)
        for k in keys:
            out("  %-68s %10.1f us   [%10.1f .. %10.1f]" % (labels[k], medians[-1][k], min(t[k]), max(t[k])))
        out("  %-68s %10.1f us" % (labels["batch"], batch_us))
        del h

    def med(k):
        return float(np.median([m[k] for m in medians]))

    def spread(k):
        return float(max(m[k] for m in medians) - min(m[k] for m in medians))

    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k in labels:
        out("  %-68s %10.1f us   spread %8.1f us" % (labels[k], med(k), spread(k)))
    out()
    pairs = F * N_CANDIDATES * (2 * WINDOW + 1) ** 2
    wins, loses = [], []
    for ci, (name, n_maps, mof) in enumerate(cases):
        # the floor of a difference in this case: the spread between runs of either path, or the distance of path 1 from its A/A twin
        twin = abs(med(("grid", ci, 1)) - med(("grid", ci, "1 again")))
        for what in ("obstacles", "grid"):
            p1, p2 = med((what, ci, 1)), med((what, ci, 2))
            floor = max(spread((what, ci, 1)), spread((what, ci, 2)), twin)
            line = "pwpp_match_%s %s: staged %.1f us, global %.1f us: global - staged = %.1f us against a floor of %.1f us (A/A distance %.1f us)" % (
                what, name, p2, p1, p1 - p2, floor, twin)
            if what == "obstacles":
                line += "; the match alone (global - visibility %.1f us, spread %.1f) %.1f us" % (med("visibility"), spread("visibility"), p1 - med("visibility"))
            else:
                line += "; %.2f ns per (frame, candidate, shift) global, %.2f staged" % (p1 * 1e3 / pairs, p2 * 1e3 / pairs)
            out(line)
            if p1 - p2 > floor:
                wins.append("pwpp_match_%s %s" % (what, name[:3]))
            if p2 - p1 > floor:
                loses.append("pwpp_match_%s %s" % (what, name[:3]))
    out()
    out("staging beats global reads by more than the floor in: " + ("; ".join(wins) if wins else "no case"))
    out("staging loses to global reads by more than the floor in: " + ("; ".join(loses) if loses else "no case"))
    out("kMatchDefaultStage (what \"match_path\" = 0 means) should be: %s" % ("true" if wins and not loses else "false"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
