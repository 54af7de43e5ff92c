"""What the line-of-sight free space (pwpp_visibility_obstacles) costs on one MI355X (profiles/obstacle_visibility_cost.txt), and the
A/B of the option "visibility_path": "0" a bit image of the frame, in LDS where it fits, "1" no bit image and no LDS, every test
of a cell reads count in global memory.

  * pwpp_visibility_obstacles of `frames` replayed KITTI frames in device memory (first, occupancy, count), band [0.2, 2.5] m,
    min_count 1, origin {0, 0}, on two grids -- 256 x 256 cells of 0.5 m and 64 x 64 cells of 2 m -- unlimited and at max_range 40
    cells, on both paths.
  * The yardstick: pwpp_rasterize_obstacles (count alone) on the same handle and grid.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), so that a drift of the
  clocks hits every variant alike.  One measurement = `reps` calls enqueued back to back and one synchronise, timed with the host
  clock and divided by `reps`: the handle's stream is its own, so no HIP event of this tool can bracket work on it.  The whole
  set is run `runs` times in this process (fresh handles each time): the spread BETWEEN runs is what a difference between the two
  paths has to exceed to be a difference.  The condition the tool states at the end: the default path is not slower than path 1
  by more than that spread in any of the four configurations.

    python tools/obstacle_visibility_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
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

GRIDS = [(256, 256, 0.5), (64, 64, 2.0)]  # (nx, ny, cell)
RADII = (0, 40)
BAND = (0.2, 2.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_visibility_cost.txt"))
    a = ap.parse_args()
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    src, kind = bench.load_source_frames("kitti")
    F = a.frames
    big, ptrs, ns, _ = device_batch(src, F, "row4")
    cells = F * max(nx * ny for nx, ny, _ in GRIDS)
    d_first, d_count = (torch.empty(cells, dtype=torch.int32, device="cuda") for _ in range(2))
    d_occ = torch.empty(cells, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()

    def timed(enqueue, sync):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            enqueue()
        sync()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    names, medians, head = None, [], False
    for run in range(a.runs):
        h = pwpp_hip.Handle()
        h.submit_batch(ptrs, ns, 4, pwpp_hip.LAYOUT_ROW_MAJOR, pwpp_hip.MEM_DEVICE, pwpp_hip.MODE_FRESH)
        h.synchronize()
        batch_us = h.time_us()

        def visibility(grid, max_range, path):
            nx, ny, cell = grid

            def go():
                h.set_option("visibility_path", path)
                return timed(lambda: h.visibility_obstacles_device(-0.5 * nx * cell, -0.5 * ny * cell, cell, nx, ny, BAND[0], BAND[1], (0.0, 0.0), 1, max_range,
                                                                   d_first.data_ptr(), d_occ.data_ptr(), d_count.data_ptr(), 0, F),
                             h.synchronize)
            return go

        def raster(grid):
            nx, ny, cell = grid
            return lambda: timed(lambda: h.rasterize_obstacles_device(-0.5 * nx * cell, -0.5 * ny * cell, cell, nx, ny, BAND[0], BAND[1], d_count.data_ptr(),
                                                                      0, 0, 0, F), h.synchronize)

        variants = []
        for g in GRIDS:
            for r in RADII:
                for path in (0, 1):
                    variants.append(("%d x %d of %.1f m, max_range %2d, path %d" % (g[0], g[1], g[2], r, path), visibility(g, r, path)))
        variants += [("%d x %d of %.1f m, pwpp_rasterize_obstacles (count) alone" % g, raster(g)) for g in GRIDS]
        t = [[] for _ in variants]
        for r in range(a.warmup + a.steps):
            for k, (_, go) in enumerate(variants):
                v = go()
                if r >= a.warmup:
                    t[k].append(v)
        if not head:
            head = True
            out("obstacle_visibility_cost: %s, %d frames, band [%.1f, %.1f] m, min_count 1, origin {0, 0}, %s" % (kind, F, BAND[0], BAND[1], torch.cuda.get_device_name(0)))
            for nx, ny, cell in GRIDS:
                h.set_option("visibility_path", 0)
                h.visibility_obstacles_device(-0.5 * nx * cell, -0.5 * ny * cell, cell, nx, ny, BAND[0], BAND[1], (0.0, 0.0), 1, 0, d_first.data_ptr(),
                                              d_occ.data_ptr(), d_count.data_ptr(), 0, F)
                h.synchronize()
                n = F * nx * ny
                occ = d_occ[:n]
                share = [100.0 * int((occ == v).sum().item()) / n for v in (pwpp_hip.OCC_OCCUPIED, pwpp_hip.OCC_FREE, pwpp_hip.OCC_UNKNOWN)]
                out("  %d x %d cells of %.1f m: %.1f %% of the cells occupied, %.1f %% free, %.1f %% unknown" % (nx, ny, cell, share[0], share[1], share[2]))
            out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds after %d warm-up rounds;"
                % (a.reps, a.steps, a.warmup))
            out("%d runs of the whole set, each with a fresh handle and batch" % a.runs)
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-62s %10.1f us   [%10.1f .. %10.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-62s %10.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-62s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    slower = []
    for gi, g in enumerate(GRIDS):
        rast = float(np.median(m[:, 8 + gi]))
        for ri, r in enumerate(RADII):
            k0 = gi * 4 + ri * 2
            p0, p1 = float(np.median(m[:, k0])), float(np.median(m[:, k0 + 1]))
            spread = max(float(m[:, k0].max() - m[:, k0].min()), float(m[:, k0 + 1].max() - m[:, k0 + 1].min()))
            out("%d x %d of %.1f m, max_range %2d: path 0 %.1f us = %.2f x the raster, path 1 %.1f us = %.2f x: path 1 - path 0 = %.1f us against a spread "
                "between runs of %.1f us; the visibility alone (path 0 - raster) %.1f us" % (g[0], g[1], g[2], r, p0, p0 / rast, p1, p1 / rast, p1 - p0, spread, p0 - rast))
            if p0 > p1 + spread:
                slower.append("%d x %d, max_range %d" % (g[0], g[1], r))
    out()
    out("the default path (0) is not slower than path 1 by more than the spread between runs in any configuration" if not slower else
        "THE DEFAULT PATH IS SLOWER THAN PATH 1 in: " + "; ".join(slower))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
