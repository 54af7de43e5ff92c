"""What the terrain analysis (pwpp_terrain_grid, pwpp_terrain_ground) costs on one MI355X (profiles/terrain_cost.txt), and the A/B of
the option "terrain_path": "1" the yardstick, every lane walks its whole (2r+1)^2 window in LDS; "2" separable, the sums of every
row over dx first, then 2r+1 rows combined with their dy.  What "0" means per radius (kTerrainDefaultSeparable, pwpp_terrain.hip)
follows from the last lines of the output.

  * `frames` replayed KITTI frames in device memory, their elevation images on 256 x 256 cells of 0.5 m; every output is a device
    array.
  * pwpp_terrain_grid alone on the device images a pwpp_rasterize_ground call left, at r = 1, 2, 3 and 4, with all five outputs and
    with cost alone: path 1, path 1 again (the A/A twin: the same variant under another name, whose distance from the first is the
    floor no difference can be read below) and path 2.
  * pwpp_terrain_ground with all five outputs on both paths, the per-frame images kept in the handle's buffer, and
    pwpp_rasterize_ground alone on the same handle and grid in the same rounds: the operator's own cost is the difference.
  Beside each time of pwpp_terrain_grid: the algorithmic bytes -- 4 in and 14 (all five) or 1 (cost alone) out per cell -- and the
  share of the HBM peak (8.0 TB/s) they amount to in that time.
  Every figure is the median over `steps` rounds; a round runs each variant once, in turn (interleaved), every other round in
  reversed order, so that a drift of the clocks and the neighbour a variant runs after hit every variant alike.  One measurement =
  `reps` calls enqueued back to back and one synchronise, timed with the host clock and divided by `reps`.  The whole set is run
  `runs` times in this process (fresh handles each time).  The floor of a case: the larger of |path 1 - its twin| and the spread of
  the three variants' medians between runs.  Path 0 becomes path 2 at a radius only where path 2 beats path 1 by more than the floor
  in BOTH output cases of that radius.

    python tools/terrain_cost.py [--frames 1024] [--steps 7] [--warmup 2] [--reps 4] [--runs 3]
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
RADII = (1, 2, 3, 4)
LIMITS = (0.2, 0.3, 0.05)
HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_cost.txt"))
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
    d_h = torch.empty(F * per, dtype=torch.float32, device="cuda")
    d_step, d_slope, d_rough = (torch.empty(F * per, dtype=torch.float32, device="cuda") for _ in range(3))
    d_count, d_cost = torch.empty(F * per, dtype=torch.uint8, device="cuda"), torch.empty(F * per, dtype=torch.int8, device="cuda")
    torch.cuda.synchronize()
    outputs = [("all five outputs", [d_step.data_ptr(), d_slope.data_ptr(), d_rough.data_ptr(), d_count.data_ptr(), d_cost.data_ptr()], 18),
               ("cost alone", [0, 0, 0, 0, d_cost.data_ptr()], 5)]
    params = {r: pwpp_hip.TerrainParams(r, 3, LIMITS[0], LIMITS[1], LIMITS[2], 0) for r in RADII}
    cases = [(r, name, p, bytes_per_cell) for r in RADII for name, p, bytes_per_cell in outputs]

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

        def raster():
            return timed(lambda: h.rasterize_ground_device(x0, y0, CELL, NX, NY, d_h.data_ptr(), 0, 0, F), h.synchronize)

        def grid(r, p, path):
            def go():
                h.set_option("terrain_path", path)
                return timed(lambda: h.terrain_grid_device(NX, NY, F, CELL, d_h.data_ptr(), params[r], *p), h.synchronize)
            return go

        def ground(r, path):
            def go():
                h.set_option("terrain_path", path)
                return timed(lambda: h.terrain_ground_device(x0, y0, CELL, NX, NY, params[r], *(outputs[0][1] + [0, 0, F])), h.synchronize)
            return go

        raster()  # (d_h holds the frames' elevation images from here on: what pwpp_terrain_grid reads)
        variants = []
        for r, name, p, _ in cases:
            for label, path in (("path 1", 1), ("path 1 twin", 1), ("path 2", 2)):
                variants.append(("pwpp_terrain_grid r %d, %s, %s" % (r, name, label), grid(r, p, path)))
        for r in RADII:
            for path in (1, 2):
                variants.append(("pwpp_terrain_ground r %d, all five outputs, path %d" % (r, path), ground(r, path)))
        variants.append(("pwpp_rasterize_ground (height) alone", raster))
        t = [[] for _ in variants]
        for rnd in range(a.warmup + a.steps):
            order = range(len(variants)) if rnd % 2 == 0 else range(len(variants) - 1, -1, -1)
            for k in order:
                v = variants[k][1]()
                if rnd >= a.warmup:
                    t[k].append(v)
        if not head:
            head = True
            out("terrain_cost: %s, %d frames, elevation images of %d x %d cells of %.1f m, %s" % (kind, F, NX, NY, CELL, torch.cuda.get_device_name(0)))
            out("min_known 3, limits %s (step m, slope, rough m)" % (LIMITS,))
            out("  the frames: %.1f %% of the cells have a height" % (100.0 * int(torch.isfinite(d_h).sum().item()) / (F * per)))
            for r in RADII:
                grid(r, outputs[0][1], 1)()
                out("  r %d: %.1f %% of the cells have a cost, %.1f %% of those 100" % (r, 100.0 * int((d_cost >= 0).sum().item()) / (F * per),
                                                                                     100.0 * int((d_cost == 100).sum().item()) / max(1, int((d_cost >= 0).sum().item()))))
            out("us per call: host clock over %d calls enqueued back to back + one synchronise; median of %d interleaved rounds (every other one reversed)"
                % (a.reps, a.steps))
            out("after %d warm-up rounds; %d runs of the whole set, each with a fresh handle and batch" % (a.warmup, a.runs))
            out()
        names = [v[0] for v in variants]
        medians.append([float(np.median(x)) for x in t] + [batch_us])
        out("run %d (min .. max of the rounds in brackets):" % run)
        for name, x in zip(names, t):
            out("  %-64s %10.1f us   [%10.1f .. %10.1f]" % (name, float(np.median(x)), min(x), max(x)))
        out("  %-64s %10.1f us" % ("the batch's own pwpp_get_time_us", batch_us))
        del h
    m = np.array(medians)
    out()
    out("over the %d runs: median of the runs' medians, and their spread (max - min) between runs" % a.runs)
    for k, name in enumerate(names + ["the batch's own pwpp_get_time_us"]):
        out("  %-64s %10.1f us   spread %8.1f us" % (name, float(np.median(m[:, k])), float(m[:, k].max() - m[:, k].min())))
    out()
    med = lambda k: float(np.median(m[:, k]))
    spread = lambda k: float(m[:, k].max() - m[:, k].min())
    ras = med(len(names) - 1)
    wins = {r: [] for r in RADII}
    for ci, (r, name, p, bytes_per_cell) in enumerate(cases):
        k1, kt, k2 = 3 * ci, 3 * ci + 1, 3 * ci + 2
        floor = max(abs(med(k1) - med(kt)), spread(k1), spread(kt), spread(k2))
        algo = bytes_per_cell * per * F
        best = min(med(k1), med(k2))
        rate = algo / (best * 1e-6)
        out("pwpp_terrain_grid r %d, %s: path 1 %.1f us, its twin %.1f us, path 2 %.1f us: path 1 - path 2 = %.1f us against a floor of %.1f us; "
            "algorithmic bytes %.1f MB = %.3f TB/s = %.2f %% of the HBM peak of %.1f TB/s on the faster path"
            % (r, name, med(k1), med(kt), med(k2), med(k1) - med(k2), floor, algo / 1e6, rate / 1e12, 100.0 * rate / HBM_PEAK, HBM_PEAK / 1e12))
        wins[r].append(med(k1) - med(k2) > floor)
    base = 3 * len(cases)
    for i, r in enumerate(RADII):
        g1, g2 = base + 2 * i, base + 2 * i + 1
        out("pwpp_terrain_ground r %d, all five outputs: path 1 %.1f us, path 2 %.1f us; pwpp_rasterize_ground alone %.1f us (spread %.1f): "
            "the operator on top of it %.1f us (path 1), %.1f us (path 2)" % (r, med(g1), med(g2), ras, spread(len(names) - 1), med(g1) - ras, med(g2) - ras))
    out()
    for r in RADII:
        out("r %d: path 2 beats path 1 by more than the floor in %d of %d output cases: kTerrainDefaultSeparable[%d] should be %s"
            % (r, sum(wins[r]), len(wins[r]), r, "true" if all(wins[r]) else "false"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del big


if __name__ == "__main__":
    main()
