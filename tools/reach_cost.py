"""What the cost-to-reach field (pwpp_reach_grid, pwpp_reach_ground) costs on one MI355X (profiles/reach_cost.txt), and the A/B of the
option "reach_path": "1" the yardstick, a workgroup per frame sweeping the frame's cells in global memory; "2" a workgroup per frame
relaxing the frame's tiles in LDS, dirty tiles revisited.  What "0" means (kReachDefaultTiled, pwpp_reach.hip) follows from the last
lines of the output.

  * `frames` replayed KITTI frames in device memory; their terrain cost bytes at radius 1 (pwpp_terrain_ground) on 256 x 256 cells of
    0.5 m and on 64 x 64 cells of 2 m; every image is a device array.  The source is the sensor's cell.
  * pwpp_reach_grid alone on those bytes, reach and from: path 1, path 1 again (the A/A twin: the same variant under another name,
    whose distance from the first is the floor no difference can be read below) and path 2; max_reach unlimited, and at the value
    of a radius of 20 m on free ground (10 * base * 20 / cell).
  * a single frame of 256 x 256 cells on both paths: one workgroup.
  * pwpp_reach_ground (256 x 256, unlimited) on both paths and pwpp_terrain_ground for its cost alone on the same handle and grid in
    the same rounds: the operator's own cost is the difference.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in
  reversed order, so that a drift of the clocks and the neighbour a variant runs after hit every variant alike.  One measurement =
  `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided by `reps` -- 16 times as many calls
  for the 64 x 64 shape, whose calls take 0.1 to 2 ms, so that a timed window is never shorter than a few milliseconds.  The output
  begins with the command line it was made with.  The whole set is run
  `runs` times in this process (fresh handles each time).  The floor of a case: the larger of |path 1 - its twin| and the spread of
  the three variants' medians between runs.  Path 0 becomes path 2 for a shape only where path 2 beats path 1 by more than the floor
  in BOTH max_reach cases of that shape, and it must never be slower than path 1 beyond the floor.

    python tools/reach_cost.py [--frames 1024] [--steps 5] [--warmup 1] [--reps 2] [--runs 2]
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

SHAPES = ((256, 0.5), (64, 2.0))  # (cells a side, metres a cell)
LIMITS = (0.2, 0.3, 0.05)
BASE, LETHAL, UNKNOWN = 10, 100, 50
RADIUS_M = 20.0
SMALL_REPS = 16  # times --reps for the shapes below 256 cells a side


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    n_max = max(n for n, _ in SHAPES)
    d_cost = {n: torch.empty(F * n * n, dtype=torch.int8, device="cuda") for n, _ in SHAPES}
    d_reach, d_from = (torch.empty(F * n_max * n_max, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    tp = pwpp_hip.TerrainParams(1, 3, LIMITS[0], LIMITS[1], LIMITS[2], 0)
    limit = {n: int(10 * BASE * RADIUS_M / cell) for n, cell in SHAPES}
    rp = lambda max_reach: pwpp_hip.ReachParams(BASE, LETHAL, UNKNOWN, 0, max_reach, 0)

    def timed(enqueue, sync, reps=None):
        reps = reps or a.reps
        t0 = time.perf_counter()
        for _ in range(reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / reps

    reps_of = lambda n: a.reps * (SMALL_REPS if n < 256 else 1)

    names, medians, head = None, [], False
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()

        def terrain(n, cell):  # (cost alone; the heights kept in the handle's buffer)
            x0 = -0.5 * n * cell
            return timed(lambda: h.terrain_ground_device(x0, x0, cell, n, n, tp, 0, 0, 0, 0, d_cost[n].data_ptr(), 0, 0, F), h.synchronize)

        def grid(n, frames, max_reach, path):
            def go():
                h.set_option("reach_path", path)
                return timed(lambda: h.reach_grid_device(n, n, frames, d_cost[n].data_ptr(), (n // 2, n // 2), rp(max_reach), d_reach.data_ptr(), d_from.data_ptr()),
                             h.synchronize, reps_of(n))
            return go

        def ground(n, cell, path):
            def go():
                h.set_option("reach_path", path)
                x0 = -0.5 * n * cell
                return timed(lambda: h.reach_ground_device(x0, x0, cell, n, n, tp, rp(0), (0.0, 0.0), d_reach.data_ptr(), d_from.data_ptr(), 0, 0, F), h.synchronize)
            return go

        for n, cell in SHAPES:
            terrain(n, cell)  # (d_cost[n] holds the frames' cost bytes from here on: what pwpp_reach_grid reads)
        variants, cases = [], []
        for n, cell in SHAPES:
            for what, max_reach in (("unlimited", 0), ("max_reach %d (%g m)" % (limit[n], RADIUS_M), limit[n])):
                cases.append((n, what))
                for label, path in (("path 1", 1), ("path 1 twin", 1), ("path 2", 2)):
                    variants.append(("pwpp_reach_grid %d x %d, %s, %s" % (n, n, what, label), grid(n, F, max_reach, path)))
        n0, cell0 = SHAPES[0]
        for path in (1, 2):
            variants.append(("pwpp_reach_grid %d x %d, ONE frame, unlimited, path %d" % (n0, n0, path), grid(n0, 1, 0, path)))
        for path in (1, 2):
            variants.append(("pwpp_reach_ground %d x %d, unlimited, path %d" % (n0, n0, path), ground(n0, cell0, path)))
        variants.append(("pwpp_terrain_ground %d x %d (cost) alone" % (n0, n0), lambda: terrain(n0, cell0)))
        t = [[] for _ in variants]
        for rnd in range(a.warmup + a.steps):
            order = range(len(variants)) if rnd % 2 == 0 else range(len(variants) - 1, -1, -1)
            for k in order:
                v = variants[k][1]()
                if rnd >= a.warmup:
                    t[k].append(v)
            print("run %d, round %d of %d done" % (run, rnd + 1, a.warmup + a.steps), file=sys.stderr, flush=True)
        if not head:
            head = True
            out("python tools/reach_cost.py --frames %d --steps %d --warmup %d --reps %d --runs %d" % (F, a.steps, a.warmup, a.reps, a.runs))
            out("reach_cost: %s, %d frames, %s" % (kind, F, torch.cuda.get_device_name(0)))
            out("terrain cost at radius 1, min_known 3, limits %s; reach: base %d, lethal %d, unknown %d; the source is the sensor's cell" % (LIMITS, BASE, LETHAL, UNKNOWN))
            for n, cell in SHAPES:
                c = d_cost[n]
                for what, max_reach in (("unlimited", 0), ("max_reach %d" % limit[n], limit[n])):
                    grid(n, F, max_reach, 1)()
                    r = d_reach[:F * n * n]
                    got = r != pwpp_hip.REACH_NONE
                    out("  %d x %d cells of %.1f m: %.1f %% of the cells have a cost, %.1f %% are lethal; %s: %.1f %% are reached, the dearest at %d"
                        % (n, n, cell, 100.0 * int((c >= 0).sum().item()) / c.numel(), 100.0 * int((c >= LETHAL).sum().item()) / c.numel(), what,
                           100.0 * int(got.sum().item()) / r.numel(), int(r[got].max().item())))
            out("us per call: host clock over %d calls (%d for the shapes below 256 cells a side) enqueued back to back + one synchronise; median of %d "
                "interleaved rounds (every other one reversed)" % (a.reps, a.reps * SMALL_REPS, a.steps))
            out("after %d warm-up rounds; %d runs of the whole set, each with a fresh handle and batch" % (a.warmup, a.runs))
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-72s %12.1f us   [%12.1f .. %12.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-72s %12.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-72s %12.1f us   spread %10.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    med = lambda k: float(np.median(m[:, k]))
    spread = lambda k: float(m[:, k].max() - m[:, k].min())
    wins = {n: [] for n, _ in SHAPES}
    for ci, (n, what) in enumerate(cases):
        k1, kt, k2 = 3 * ci, 3 * ci + 1, 3 * ci + 2
        floor = max(abs(med(k1) - med(kt)), spread(k1), spread(kt), spread(k2))
        out("pwpp_reach_grid %d x %d, %s: path 1 %.1f us, its twin %.1f us, path 2 %.1f us: path 1 - path 2 = %.1f us against a floor of %.1f us; "
            "%.2f us a frame on the faster path" % (n, n, what, med(k1), med(kt), med(k2), med(k1) - med(k2), floor, min(med(k1), med(k2)) / F))
        wins[n].append(med(k1) - med(k2) > floor)
    base = 3 * len(cases)
    out("pwpp_reach_grid %d x %d, ONE frame (one workgroup): path 1 %.1f us, path 2 %.1f us" % (n0, n0, med(base), med(base + 1)))
    ter = med(base + 4)
    out("pwpp_reach_ground %d x %d, unlimited: path 1 %.1f us, path 2 %.1f us; pwpp_terrain_ground (cost) alone %.1f us (spread %.1f): "
        "the operator on top of it %.1f us (path 1), %.1f us (path 2)" % (n0, n0, med(base + 2), med(base + 3), ter, spread(base + 4), med(base + 2) - ter, med(base + 3) - ter))
    out()
    for n, _ in SHAPES:
        out("%d x %d: path 2 beats path 1 by more than the floor in %d of %d max_reach cases: path 0 should be path %d there"
            % (n, n, sum(wins[n]), len(wins[n]), 2 if all(wins[n]) else 1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
