"""What the costmap (pwpp_costmap_grid, pwpp_costmap_obstacles) costs on one MI355X (profiles/costmap_cost.txt), and the A/B of the option
"costmap_path": "1" the yardstick, a lane per cell with the inflation curve read from global memory; "2" the curve staged once per
workgroup into LDS, four consecutive cells a lane.  What "0" means (PWPP_COSTMAP_QUADS_FROM_CELLS, pwpp_costmap.h) follows from the last
lines of the output.

  * `frames` replayed KITTI frames in device memory; on 256 x 256 cells of 0.5 m, 128 x 128 of 1 m and 64 x 64 of 2 m their visibility bytes
    (pwpp_visibility_obstacles), their uncapped obstacle distances (pwpp_distance_obstacles) and their terrain cost bytes at radius 1
    (pwpp_terrain_ground): every image is a device array.
  * pwpp_costmap_grid alone on those images, all three layers, cost and why, with a short curve (pwpp_costmap_curve: inscribed 0.6 m,
    radius 3 m) and with the longest (4097 entries): path 1, path 1 again (the A/A twin: the same variant under another name, whose
    distance from the first is the floor no difference can be read below) and path 2.  Its algorithmic bytes -- 1 + 1 + 4 read, 1 + 1
    written per cell -- over the time, as a share of the HBM peak.
  * pwpp_costmap_grid without a dist2 image (256 x 256, the short curve): the widening and the capped distances inside the call.
  * pwpp_costmap_obstacles (256 x 256, the short curve, every layer) on both paths, and its stages as stand-alone calls on the same
    handle and grid in the same rounds: pwpp_visibility_obstacles, pwpp_distance_obstacles with the same cap, pwpp_terrain_ground for
    its cost alone, and pwpp_rasterize_obstacles: the chain rasterises the obstacles once where the two stand-alone calls do it twice.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in
  reversed order.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided by
  `reps` -- 16 times as many calls for the shapes below 256 cells a side.  The whole set is run `runs` times in this process (fresh handles each time).
  The floor of a case: the larger of |path 1 - its twin| and the spread of the three variants' medians between runs.  Path 0 becomes
  path 2 only where it wins: from the cells of the smallest shape at and above which path 2 beats path 1 by more than the floor with
  both curves; below that the yardstick stays.

    python tools/costmap_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 2]
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

SHAPES = ((256, 0.5), (128, 1.0), (64, 2.0))  # (cells a side, metres a cell): 2^26, 2^24 and 2^22 cells a call of 1024 frames
LIMITS = (0.2, 0.3, 0.05)
BAND = (0.3, 2.5)
MAX_RANGE = 0
SMALL_REPS = 16  # times --reps for the shapes below 256 cells a side
HBM_PEAK = 8.0e12  # bytes/s (MI355X)
CELL_BYTES = 1 + 1 + 4 + 1 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "costmap_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    n_max = max(n for n, _ in SHAPES)
    d_occ, d_ter = ({n: torch.empty(F * n * n, dtype=torch.int8, device="cuda") for n, _ in SHAPES} for _ in range(2))
    d_dist = {n: torch.empty(F * n * n, dtype=torch.int32, device="cuda") for n, _ in SHAPES}
    d_first = torch.empty(F * n_max * n_max, dtype=torch.int32, device="cuda")
    d_cost, d_why, d_cost2, d_why2 = (torch.empty(F * n_max * n_max, dtype=torch.int8, device="cuda") for _ in range(4))
    torch.cuda.synchronize()
    tp = pwpp_hip.TerrainParams(1, 3, LIMITS[0], LIMITS[1], LIMITS[2], 0)
    cp = pwpp_hip.CostmapParams(7, -1, -1, 100)
    curves = {n: {"short": pwpp_hip.costmap_curve(cell, 0.6, 3.0, 1.5, 99), "4097": np.minimum(100, np.arange(4097)[::-1] // 40).astype(np.uint8)} for n, cell in SHAPES}

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
        geo = lambda n, cell: (-0.5 * n * cell, -0.5 * n * cell, cell, n, n)

        def visibility(n, cell):
            return timed(lambda: h.visibility_obstacles_device(*geo(n, cell), BAND[0], BAND[1], (0.0, 0.0), 1, MAX_RANGE, d_first.data_ptr(), d_occ[n].data_ptr(), 0, 0, F),
                         h.synchronize)

        def distance(n, cell, max_dist, into):
            return timed(lambda: h.distance_obstacles_device(*geo(n, cell), BAND[0], BAND[1], 1, max_dist, into.data_ptr(), 0, 0, 0, 0, F), h.synchronize)

        def terrain(n, cell):  # (cost alone; the heights kept in the handle's buffer)
            return timed(lambda: h.terrain_ground_device(*geo(n, cell), tp, 0, 0, 0, 0, d_ter[n].data_ptr(), 0, 0, F), h.synchronize)

        def grid(n, curve, path, own=False):
            def go():
                h.set_option("costmap_path", path)
                return timed(lambda: h.costmap_grid_device(n, n, F, cp, d_cost.data_ptr(), d_occ[n].data_ptr(), d_ter[n].data_ptr(), 0 if own else d_dist[n].data_ptr(),
                                                           curves[n][curve], d_why.data_ptr()), h.synchronize, reps_of(n))
            return go

        def chain(n, cell, path):
            def go():
                h.set_option("costmap_path", path)
                return timed(lambda: h.costmap_obstacles_device(*geo(n, cell), cp, d_cost2.data_ptr(), BAND[0], BAND[1], 1, (0.0, 0.0), MAX_RANGE, tp, curves[n]["short"],
                                                                d_why2.data_ptr(), 0, 0, 0, 0, F), h.synchronize)
            return go

        for n, cell in SHAPES:  # (the layers' images hold the frames' bytes from here on: what pwpp_costmap_grid reads)
            visibility(n, cell), distance(n, cell, 0, d_dist[n]), terrain(n, cell)
        variants, cases = [], []
        for n, cell in SHAPES:
            for curve in ("short", "4097"):
                cases.append((n, curve))
                for label, path in (("path 1", 1), ("path 1 twin", 1), ("path 2", 2)):
                    variants.append(("pwpp_costmap_grid %d x %d, curve %s (%d), %s" % (n, n, curve, len(curves[n][curve]), label), grid(n, curve, path)))
        n0, cell0 = SHAPES[0]
        cap0 = 1
        while cap0 * cap0 < len(curves[n0]["short"]) - 1:
            cap0 += 1
        variants.append(("pwpp_costmap_grid %d x %d, own distances (cap %d), path 0" % (n0, n0, cap0), grid(n0, "short", 0, own=True)))
        for path in (1, 2):
            variants.append(("pwpp_costmap_obstacles %d x %d, every layer, path %d" % (n0, n0, path), chain(n0, cell0, path)))
        d_near = d_first  # (an int32 image nobody reads)
        variants.append(("pwpp_visibility_obstacles %d x %d alone" % (n0, n0), lambda: visibility(n0, cell0)))
        variants.append(("pwpp_distance_obstacles %d x %d, max_dist %d, alone" % (n0, n0, cap0), lambda: distance(n0, cell0, cap0, d_near)))
        variants.append(("pwpp_terrain_ground %d x %d (cost) alone" % (n0, n0), lambda: terrain(n0, cell0)))
        variants.append(("pwpp_rasterize_obstacles %d x %d (count) alone" % (n0, n0), lambda: timed(
            lambda: h.rasterize_obstacles_device(*geo(n0, cell0), BAND[0], BAND[1], d_near.data_ptr(), 0, 0, 0, F), h.synchronize)))
        t = [[] for _ in variants]
        for rnd in range(a.warmup + a.steps):
            order = range(len(variants)) if rnd % 2 == 0 else range(len(variants) - 1, -1, -1)
            for k in order:
                v = variants[k][1]()
                if rnd >= a.warmup:
                    t[k].append(v)
            print("run %d, round %d of %d done" % (run, rnd + 1, a.warmup + a.steps), file=sys.stderr, flush=True)
        h.set_option("costmap_path", 0)
        if not head:
            head = True
            out("python tools/costmap_cost.py --frames %d --steps %d --warmup %d --reps %d --runs %d" % (F, a.steps, a.warmup, a.reps, a.runs))
            out("costmap_cost: %s, %d frames, %s" % (kind, F, torch.cuda.get_device_name(0)))
            out("height band %s m, min_count 1, max_range unlimited, terrain at radius 1 with limits %s; layers 7, unknowns stay unknown, unknown_below 100" % (BAND, LIMITS))
            for n, cell in SHAPES:
                grid(n, "short", 1)()
                c, w = d_cost[:F * n * n], d_why[:F * n * n]
                grid(n, "short", 2)()
                out("  %d x %d cells of %.1f m: occupied %.2f %%, free %.1f %%, terrain known %.1f %%; cost: unknown %.1f %%, lethal %.2f %%, 1 .. 99 %.1f %%; "
                    "named by the inflation %.2f %%" % (n, n, cell, 100.0 * (d_occ[n] == 100).float().mean().item(), 100.0 * (d_occ[n] == 0).float().mean().item(),
                                                       100.0 * (d_ter[n] >= 0).float().mean().item(), 100.0 * (c == -1).float().mean().item(),
                                                       100.0 * (c == 100).float().mean().item(), 100.0 * ((c > 0) & (c < 100)).float().mean().item(),
                                                       100.0 * ((w & 2) != 0).float().mean().item()))
            own = grid(n0, "short", 0, own=True)
            grid(n0, "short", 0)()
            keep = d_cost[:F * n0 * n0].clone()
            own()
            out("  own distances give the bytes of the supplied uncapped image: %s" % bool((keep == d_cost[:F * n0 * n0]).all().item()))
            chain(n0, cell0, 0)()
            out("  the chain gives the bytes of pwpp_costmap_grid on the stages' images: %s" % bool((keep == d_cost2[:F * n0 * n0]).all().item()))
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
    wins, losses = [], []
    for ci, (n, curve) in enumerate(cases):
        k1, kt, k2 = 3 * ci, 3 * ci + 1, 3 * ci + 2
        floor = max(abs(med(k1) - med(kt)), spread(k1), spread(kt), spread(k2))
        best = min(med(k1), med(k2))
        out("pwpp_costmap_grid %d x %d, curve %s: path 1 %.1f us, its twin %.1f us, path 2 %.1f us: path 1 - path 2 = %.1f us against a floor of %.1f us; "
            "the faster path moves %d algorithmic bytes a cell at %.2f TB/s, %.0f %% of the HBM peak"
            % (n, n, curve, med(k1), med(kt), med(k2), med(k1) - med(k2), floor, CELL_BYTES, F * n * n * CELL_BYTES / best * 1e-6,
               100.0 * F * n * n * CELL_BYTES / (best * 1e-6) / HBM_PEAK))
        wins.append(med(k1) - med(k2) > floor)
        losses.append(med(k2) - med(k1) > floor)
    base = 3 * len(cases)
    out("pwpp_costmap_grid %d x %d with its own distances: %.1f us (the fold alone on path 1: %.1f us)" % (n0, n0, med(base), med(0)))
    stages = med(base + 3) + med(base + 4) + med(base + 5) - med(base + 6)
    out("pwpp_costmap_obstacles %d x %d: path 1 %.1f us, path 2 %.1f us; its stages alone: visibility %.1f + distance %.1f + terrain %.1f - one of their two "
        "obstacle rasters %.1f = %.1f us: the chain on top of its stages %.1f us (path 1), %.1f us (path 2)"
        % (n0, n0, med(base + 1), med(base + 2), med(base + 3), med(base + 4), med(base + 5), med(base + 6), stages, med(base + 1) - stages, med(base + 2) - stages))
    out()
    from_cells = None
    for n, _ in sorted(SHAPES):  # the smallest shape at and above which path 2 wins with both curves
        if all(w for (m_, _c), w in zip(cases, wins) if m_ >= n):
            from_cells = F * n * n
            break
    out("path 2 beats path 1 by more than the floor in %d of %d cases and loses by more than the floor in %d" % (sum(wins), len(wins), sum(losses)))
    out("path 0 should be path 2 %s" % ("from %d cells a call (%d frames of the smallest shape it wins at), path 1 below" % (from_cells, F) if from_cells else "nowhere: path 1"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
